"""The energy score on the GPU (d3p_energy_score, d3p_amd.energy) against tests/energy_ref.py, every shape under each forced form.  The
four rows lie within the DERIVED bound of the float64 comparator (energy_ref.bound), NaN by class on exactly the flagged rows; the cases
with exact arithmetic are compared by value, which catches a dropped or doubled pair the bound would let through; everything the
contract calls independent -- position, neighbours, rows, strides, a repeat, the form -- is compared bit for bit.  `out` is filled with
0xFF bytes before every call.  The largest error-to-bound ratio is printed (pytest -s) and recorded in docs/experiments_energy.md."""
import argparse
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import energy_ref as ER
from tests import scoring_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 12345.0
ICANARY = 12345
PAD = 64
FORMS = (1, 2)
_REF = {}      # case name -> (exact, bound): computed once, shared by the forms, never changed


def np_(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module")
def LIB(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    yield lib
    assert lib.d3p_energy_score_set_form(0) == 0


@pytest.fixture(scope="module")
def TCR(LIB):
    """(T, C, R) from the query functions: items a side of a pair tile, columns of a staged chunk, rows per workgroup of the rows form."""
    return int(LIB.d3p_energy_score_tile_draws()), int(LIB.d3p_energy_score_chunk_cols()), int(LIB.d3p_energy_score_rows_per_group(1))


@pytest.fixture(params=FORMS, ids=["rows-form", "streamed-form"])
def form(request, LIB):
    assert LIB.d3p_energy_score_set_form(request.param) == 0
    yield request.param
    assert LIB.d3p_energy_score_set_form(0) == 0


def entry(z, y, pads=(0, 0, 0, 0), expect=0):
    """d3p_energy_score on the (n, rows, d) numpy tensor z against the (rows, d) y with ld_row = d + pads[0], ld_draw = rows ld_row +
    pads[1], y_ld = d + pads[2], out_ld = rows + pads[3]; canaries in every padding, `out` pre-filled with 0xFF bytes: (4, rows) float32
    after the paddings were checked."""
    import d3p_amd._lib as L
    n, rows, d = z.shape
    is_int = z.dtype == np.int32
    tdt, can = (torch.int32, ICANARY) if is_int else (torch.float32, CANARY)
    ld_row, y_ld, out_ld = d + pads[0], d + pads[2], rows + pads[3]
    ld_draw = rows * ld_row + pads[1]
    zb = torch.full((n * ld_draw + PAD,), can, dtype=tdt, device="cuda")
    zv = zb.as_strided((n, rows, d), (ld_draw, ld_row, 1))
    zv.copy_(torch.tensor(z))
    before = zb.clone()
    yb = torch.full((rows * y_ld + PAD,), can, dtype=tdt, device="cuda")
    yb.as_strided((rows, d), (y_ld, 1)).copy_(torch.tensor(np.asarray(y, z.dtype).reshape(rows, d)))
    out = torch.full((PAD + 4 * out_ld + PAD,), -1, dtype=torch.int32, device="cuda")            # 0xFF bytes
    rc = L.load().d3p_energy_score(L.stream_ptr(), L.ptr(zb), int(is_int), ld_draw, ld_row, n, rows, d, L.ptr(yb), y_ld, L.ptr(out[PAD:]), out_ld)
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.load().d3p_last_error())
    assert torch.equal(zb.view(torch.int32), before.view(torch.int32)), "the draws were written"
    body = out[PAD:PAD + 4 * out_ld].reshape(4, out_ld)
    assert bool((out[:PAD] == -1).all()) and bool((out[PAD + 4 * out_ld:] == -1).all()) and bool((body[:, rows:] == -1).all()), \
        "the scores were written outside their extent"
    if expect != 0:
        assert bool((body == -1).all()), "a refused call wrote"
        return None
    return np_(body[:, :rows].contiguous().view(torch.float32)).copy()


def data(seed, n, rows, d, is_int):
    rng = np.random.default_rng(seed)
    if is_int:
        return rng.integers(-50, 51, (n, rows, d)).astype(np.int32), rng.integers(-50, 51, (rows, d)).astype(np.int32)
    return rng.normal(size=(n, rows, d)).astype(np.float32), rng.normal(size=(rows, d)).astype(np.float32)


def reference(name, z, y):
    if name not in _REF:
        ex = ER.exact(z, y)
        _REF[name] = (ex, ER.bound(ex, z.shape[0], z.shape[2]))
    return _REF[name]


def within(got, ex, tol, n):
    """got (4, rows) float32 within tol of ex, NaN by class on exactly ex's NaNs: the largest error / bound."""
    worst = 0.0
    for i, k in enumerate(ER.NAMES):
        nan = np.isnan(ex[k])
        assert np.array_equal(np.isnan(got[i]), nan), (k, got[i], ex[k])
        if nan.all():
            continue
        err = np.abs(got[i].astype(np.float64) - ex[k])[~nan]
        ratio = err / tol[k][~nan]
        assert (ratio <= 1.0).all(), (k, float(ratio.max()), int(n))
        worst = max(worst, float(ratio.max()))
    return worst


def by_value(z, y, S1, U):
    """The four float32 an exact row must give: S1 and U are exact in float64, the closing arithmetic is the rule's."""
    got = entry(z, y, pads=(1, 3, 2, 5))
    n = z.shape[0]
    for r in range(z.shape[1]):
        want = np.array(ER._finish(S1[r], U[r], n)).astype(np.float32)
        assert np.array_equal(bits(got[:, r]), bits(want)) or (np.isnan(want[1]) and np.array_equal(bits(got[[0, 2, 3], r]), bits(want[[0, 2, 3]]))
                                                               and np.isnan(got[1, r])), (r, got[:, r], want)
    return got


# ------------------------------------------------------------------------------------------------ against the comparator
def _sweep(T, C, R):
    ns = (1, 2, 3, T - 1, T, T + 1, 2 * T + 1)
    ds = (1, 2, 3, C - 1, C, C + 1, 2 * C + 1)
    rs = (1, R - 1, R, R + 1, 3 * R + 1)
    cases = [(n, 3, R + 1) for n in ns] + [(T + 1, d, 3) for d in ds] + [(5, 2, r) for r in rs]
    cases += [(2 * T + 1, 2 * C + 1, 2), (T, C, R), (1, 1, 1), (2, C + 1, R - 1), (T + 1, 1, 3 * R + 1), (3, C - 1, R + 1)]
    return list(dict.fromkeys(cases))


def test_sweep_against_the_comparator_within_the_bound(form, TCR):
    T, C, R = TCR
    worst = 0.0
    for i, (n, d, rows) in enumerate(_sweep(T, C, R)):
        is_int = i % 2 == 1
        z, y = data(100 + i, n, rows, d, is_int)
        ex, tol = reference(f"sweep{i}", z, y)
        pads = ((0, 0, 0, 0), (1, 0, 0, 3), (0, 7, 2, 0), (5, 3, 1, 9))[i % 4]
        worst = max(worst, within(entry(z, y, pads), ex, tol, n))
    print(f"form {form}: largest error / bound over the sweep {worst:.4f}")


def test_the_vae_width_runs(form):
    n, rows, d = 8, 3, 784
    rng = np.random.default_rng(7)
    z, y = rng.integers(0, 2, (n, rows, d)).astype(np.int32), rng.integers(0, 2, (rows, d)).astype(np.int32)
    ex, tol = reference("vae", z, y)
    got = entry(z, y, pads=(0, 16, 0, 1))
    print(f"form {form}: d = 784 error / bound {within(got, ex, tol, n):.4f}")


def test_clustered_far_from_the_origin(form, TCR):
    T, C, R = TCR
    rng = np.random.default_rng(8)
    z = (1.0e4 + 1.0e-3 * rng.normal(size=(T + 3, R + 1, 2))).astype(np.float32)
    y = (1.0e4 + 1.0e-3 * rng.normal(size=(R + 1, 2))).astype(np.float32)
    ex, tol = reference("far", z, y)
    print(f"form {form}: clustered draws error / bound {within(entry(z, y), ex, tol, T + 3):.4f}")


# ------------------------------------------------------------------------------------------------ by value
def test_exact_cases_by_value(form, TCR):
    T, C, R = TCR
    rng = np.random.default_rng(9)
    # d = 1, small integers, both dtypes, n across the tile edge
    for n, dtype in ((3, np.int32), (T + 1, np.float32), (2 * T + 1, np.int32)):
        rows = R + 1
        k = rng.integers(-20, 21, (n, rows))
        ky = rng.integers(-20, 21, rows)
        S1 = np.abs(k - ky[None, :]).sum(axis=0).astype(np.float64)
        U = np.array([np.abs(k[:, r][:, None] - k[:, r][None, :]).sum() / 2 for r in range(rows)], np.float64)
        by_value(k.astype(dtype)[:, :, None], ky.astype(dtype)[:, None], S1, U)
    # d = 2, points k (3, 4): every distance is 5 |k_i - k_j|
    n, rows = T + 2, 3
    k = rng.integers(-30, 31, (n, rows))
    ky = rng.integers(-30, 31, rows)
    z = (k[:, :, None] * np.array([3, 4])).astype(np.float32)
    S1 = 5.0 * np.abs(k - ky[None, :]).sum(axis=0)
    U = np.array([5.0 * np.abs(k[:, r][:, None] - k[:, r][None, :]).sum() / 2 for r in range(rows)])
    by_value(z, (ky[:, None] * np.array([3, 4])).astype(np.float32), S1, U)
    # 0/1 int32 rows of prefix ones of lengths 0, 9, 25: the Hamming distances 9, 16, 25 are perfect squares (y: length 0, or 25)
    d = C + 8
    assert d >= 25
    m = np.array([0, 9, 25])
    z = (np.arange(d)[None, :] < m[:, None]).astype(np.int32)[:, None, :].repeat(2, axis=1)
    y = np.stack([np.zeros(d, np.int32), (np.arange(d) < 25).astype(np.int32)])
    by_value(z, y, np.array([0.0 + 3 + 5, 5.0 + 4 + 0]), np.array([3.0 + 5 + 4] * 2))
    # all draws equal: spread == 0 and es == mae;   all draws equal to y: every output is 0, es_fair too
    p = rng.normal(size=(1, 2, 5)).astype(np.float32)
    z = np.repeat(p, T + 1, axis=0)
    y = np.stack([p[0, 0] + np.float32(1.0), p[0, 1]])
    got = entry(z, y)
    assert (got[3] == 0.0).all() and np.array_equal(bits(got[0]), bits(got[2])) and np.array_equal(bits(got[1]), bits(got[2]))
    assert got[2, 0] > 0 and (got[:, 1] == 0.0).all() and not np.signbit(got[:, 1]).any()
    em = ER.emulate(z, y)
    assert got[2, 0] == em["mae"][0]
    # n = 1: es_fair is NaN, spread 0, es = mae
    z, y = data(10, 1, R + 1, 3, False)
    got = entry(z, y)
    assert np.isnan(got[1]).all() and (got[3] == 0.0).all() and np.array_equal(bits(got[0]), bits(got[2])) and (got[2] > 0).all()


def test_d1_agrees_with_the_crps(form, gpu):
    from d3p_amd import energy as E
    from d3p_amd import scoring as SC
    rng = np.random.default_rng(12)
    n, rows = 37, 21
    m = rng.normal(size=(n, rows)).astype(np.float32)
    y = rng.normal(size=rows).astype(np.float32)
    mt, yt = torch.tensor(m).cuda(), torch.tensor(y).cuda()
    got, crps = E.energy_score_draws(mt, yt), SC.score_draws(mt, yt)
    ex = ER.exact(m, y)
    tol_e, tol_s = ER.bound(ex, n, 1), SR.bound(m, y)
    for i, (ke, ks) in enumerate((("es", "crps"), ("es_fair", "crps_fair"), ("mae", "mae"), ("spread", "spread"))):
        diff = np.abs(np_(got[ke]).astype(np.float64) - np_(crps[ks]).astype(np.float64))
        assert (diff <= tol_e[ke] + tol_s[i]).all(), (ke, float((diff / (tol_e[ke] + tol_s[i])).max()))
    assert np.array_equal(bits(np_(E.energy_score(mt, yt, fair=True))), bits(np_(got["es_fair"])))
    assert np.array_equal(bits(np_(E.energy_score(mt[:, :, None], yt[:, None]))), bits(np_(got["es"])))     # the 3-D spelling of d = 1


# ------------------------------------------------------------------------------------------------ determinism
def test_a_rows_bits_depend_on_that_row_alone(LIB, TCR):
    T, C, R = TCR
    n, d = 2 * T + 3, C + 3
    z, y = data(20, n, 3 * R + 2, d, False)
    runs = {}
    for f in FORMS:
        assert LIB.d3p_energy_score_set_form(f) == 0
        base = entry(z, y)
        assert np.array_equal(bits(entry(z, y)), bits(base))                                         # a repeat call
        assert np.array_equal(bits(entry(z, y, pads=(3, 11, 5, 2))), bits(base))                     # other strides
        rows = z.shape[1]
        perm = np.random.default_rng(21).permutation(rows)                                           # other positions, other neighbours
        assert np.array_equal(bits(entry(z[:, perm], y[perm])[:, np.argsort(perm)]), bits(base))
        for keep in (1, R - 1, R + 1):                                                               # another rows, alone in its workgroup
            assert np.array_equal(bits(entry(z[:, 5:5 + keep], y[5:5 + keep])), bits(base[:, 5:5 + keep]))
        runs[f] = base
    assert LIB.d3p_energy_score_set_form(0) == 0
    assert np.array_equal(bits(runs[1]), bits(runs[2]))                                              # the forms agree bit for bit
    assert np.array_equal(bits(entry(z, y)), bits(runs[1]))                                          # and so does the rule's choice


def test_special_rows_leave_their_neighbours_alone(form, TCR):
    T, C, R = TCR
    n, rows, d = T + 1, R + 3, 3
    z, y = data(30, n, rows, d, False)
    base = entry(z, y)
    bad_z, bad_y = z.copy(), y.copy()
    bad_z[n - 1, 1, 2] = np.nan                     # a NaN draw
    bad_z[0, 4, 0] = np.inf                         # a +inf draw
    bad_y[R, 1] = -np.inf                           # a -inf observation
    bad_z[3, 7, :] = (1e30, 0.0, 0.0)               # finite, but q overflows float32 against every other item
    bad_y[9, 0] = 1e30                              # finite, but q overflows against y alone: the spread stays finite
    got = entry(bad_z, bad_y)
    special = [1, 4, R, 7, 9]
    keep = [r for r in range(rows) if r not in special]
    assert np.array_equal(bits(got[:, keep]), bits(base[:, keep]))
    assert np.isnan(got[:, [1, 4, R]]).all()
    assert got[2, 7] == np.inf and got[3, 7] == np.inf and np.isnan(got[0, 7]) and np.isnan(got[1, 7])     # IEEE from the overflow on
    assert got[2, 9] == np.inf and got[0, 9] == np.inf and got[1, 9] == np.inf
    assert np.isfinite(got[3, 9]) and bits(got[3, 9:10])[0] == bits(base[3, 9:10])[0]                      # (the spread never reads y)


# ------------------------------------------------------------------------------------------------ the Python and model layers
def test_python_layer_on_the_device(gpu):
    from d3p_amd import energy as E
    z, y = data(40, 6, 9, 4, True)
    zt = torch.tensor(z).cuda()
    want = entry(z, y)
    got = E.energy_score_draws(zt, torch.tensor(y))                                 # (y on the host is moved)
    for i, k in enumerate(ER.NAMES):
        assert got[k].shape == (9,) and got[k].dtype == torch.float32 and np.array_equal(bits(np_(got[k])), bits(want[i])), k
    assert np.array_equal(bits(np_(E.energy_score_draws(zt, torch.tensor(y).double())["es"])), bits(want[0]))   # integral floats are cast
    wide = torch.zeros((6, 12, 7), dtype=torch.int32, device="cuda")
    wide[:, :9, :4] = zt
    assert np.array_equal(bits(np_(E.energy_score(wide[:, :9, :4], torch.tensor(y)))), bits(want[0]))           # a strided view
    for v in (2 ** 24 + 1, -2 ** 24 - 1):
        big = zt.clone()
        big[2, 3, 1] = v
        with pytest.raises(ValueError, match="beyond 2\\^24"):
            E.energy_score_draws(big, torch.tensor(y))
    edge = zt.clone()
    edge[2, 3, 1] = 2 ** 24
    assert bool(torch.isfinite(E.energy_score_draws(edge, torch.tensor(y))["es"]).all())
    empty = E.energy_score_draws(torch.zeros((4, 0, 3), device="cuda"), torch.zeros((0, 3)))
    assert all(empty[k].shape == (0,) for k in ER.NAMES)


def test_model_layer_scores_the_mixtures_own_draws(gpu):
    from d3p_amd import energy as E
    from d3p_amd import mixture as MX
    from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel
    from d3p_amd.random import debug as threefry
    k, d, rows, n = 3, 2, 130, 5
    rng = np.random.default_rng(50)
    obs = torch.tensor(rng.normal(size=(rows, d)).astype(np.float32) * 2).cuda()
    params = {"alpha_log": torch.tensor(rng.normal(size=k).astype(np.float32)).cuda(),
              "mus_loc": torch.tensor(rng.normal(size=(k, d)).astype(np.float32) * 3).cuda()}
    model = GaussianMixtureModel()
    guide = GaussianMixtureGuide(model)
    key = threefry.PRNGKey(77)
    draws = MX.posterior_predictive_samples(key, n, model, (k, obs), guide, params)["obs"]
    assert draws.shape == (n, rows, d)
    want = E.energy_score_draws(draws, obs)
    res = E.posterior_predictive_energy_score(key, n, model, (k, obs), guide, params, pointwise=True)
    assert (res.n_draws, res.n_rows, res.dim) == (n, rows, d) and res.es.dtype == torch.float64
    for name in ("es", "mae", "spread"):
        assert np.array_equal(bits(np_(res.pointwise[name])), bits(np_(want[name]))), name
    es = np_(want["es"]).astype(np.float64)
    assert float(res.es) == pytest.approx(es.mean(), rel=1e-14) and float(res.se) == pytest.approx(es.std(ddof=1) / np.sqrt(rows), rel=1e-12)
    assert float(res.mae) == pytest.approx(np_(want["mae"]).astype(np.float64).mean(), rel=1e-14)
    fair = E.posterior_predictive_energy_score(key, n, model, (k, obs), guide, params, fair=True, pointwise=True)
    assert fair.pointwise is not None and np.array_equal(bits(np_(fair.pointwise["es"])), bits(np_(want["es_fair"])))
    plain = E.posterior_predictive_energy_score(key, n, model, (k, obs), guide, params)
    assert plain.pointwise is None and float(plain.es) == float(res.es)
    ex = ER.exact(np_(draws), np_(obs))
    within(np.stack([np_(want[name]) for name in ER.NAMES]), ex, ER.bound(ex, n, d), n)
    cmp = E.compare_energy_scores(res, fair)
    assert float(cmp.es_diff) == pytest.approx((es - np_(want["es_fair"]).astype(np.float64)).mean(), rel=1e-12) and float(cmp.es_diff) > 0


def test_example_flag_reports_the_energy_score(gpu, capsys):
    spec = importlib.util.spec_from_file_location("ex_gmm_energy", os.path.join(ROOT, "examples", "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = argparse.Namespace(num_epochs=2, learning_rate=5e-2, batch_size=64, dimensions=2, num_samples=512, num_components=3, sigma=0.3,
                              energy_score=4)
    mod.main(args)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("held-out energy score")]
    assert len(line) == 1
    m = re.search(r"\(mean over (\d+) points, 4 predictive draws\): ([0-9.]+) \+- ([0-9.]+) \(mean distance ([0-9.]+), spread ([0-9.]+)\)", line[0])
    assert m and int(m.group(1)) > 0
    es, se, mae, spread = (float(m.group(i)) for i in (2, 3, 4, 5))
    assert es > 0 and se > 0 and abs(es - (mae - spread)) < 2e-4
    assert mod.parse_args(["--energy-score"]).energy_score == 100 and mod.parse_args(["--energy-score", "7"]).energy_score == 7
    assert mod.parse_args([]).energy_score is None
