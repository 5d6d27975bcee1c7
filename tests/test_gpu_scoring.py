"""CRPS and PIT counts on the GPU (d3p_col_crps, d3p_amd.scoring) against tests/scoring_ref.py.  The four float rows lie within the
DERIVED bound of the comparator (scoring_ref.bound: half a float32 ulp plus (n + 8) float64 roundings of the sums' magnitudes), NaN by
class on exactly the flagged columns; the two counts are equal by value; everything the contract calls independent is compared bit for
bit.  The largest error-to-bound ratio of the sweep is printed per case (pytest -s) and recorded in docs/experiments_scoring.md."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests import loglik_ref as LR
from tests import moments_ref as MR
from tests import predictive_ref as P
from tests import scoring_ref as SR

pytestmark = pytest.mark.gpu
CANARY = 12345.0
ICANARY = 12345
PAD = 64


def np_(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module")
def SC(gpu):
    from d3p_amd import scoring
    return scoring


@pytest.fixture(scope="module")
def FORMS(gpu):
    """(N32, N8, Nmax): the largest n of the 32-column form, of the 8-column form, and d3p_col_crps_max_n(), from the query functions."""
    import d3p_amd._lib as L
    lib = L.load()
    nmax = int(lib.d3p_col_crps_max_n())

    def largest(form):
        lo, hi = 1, nmax                                  # cols_per_group falls with n: the largest n that still gives `form` or wider
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if lib.d3p_col_crps_cols_per_group(mid) >= form else (lo, mid - 1)
        assert lib.d3p_col_crps_cols_per_group(lo) == form and lib.d3p_col_crps_cols_per_group(lo + 1) < form
        return lo
    n32, n8 = largest(32), largest(8)
    assert n32 < n8 < nmax and lib.d3p_col_crps_cols_per_group(nmax) == 2 and lib.d3p_col_crps_cols_per_group(nmax + 1) == 0
    return n32, n8, nmax


def entry(m, y, ld=None, expect=0):
    """d3p_col_crps on the (n, cols) numpy matrix m at leading dimension ld against y, canaries in the matrix's padding, between the rows
    of both outputs (out_ld = counts_ld = cols + PAD) and around them: ((4, cols) float32, (2, cols) int64) after the canaries were
    checked.  expect: the return code; where it is not 0 both outputs must be untouched."""
    import d3p_amd._lib as L
    n, cols = m.shape
    ld = cols if ld is None else ld
    is_int = m.dtype == np.int32
    tdt = torch.int32 if is_int else torch.float32
    mat = torch.full((n, ld), ICANARY if is_int else CANARY, dtype=tdt, device="cuda")
    mat[:, :cols] = torch.tensor(m).cuda()
    yt = torch.tensor(np.asarray(y, m.dtype)).cuda()
    old = cols + PAD
    out = torch.full((PAD + 4 * old + PAD,), CANARY, device="cuda")
    cnt = torch.full((PAD + 2 * old + PAD,), ICANARY, dtype=torch.int32, device="cuda")
    rc = L.load().d3p_col_crps(L.stream_ptr(), L.ptr(mat), int(is_int), ld, n, cols, L.ptr(yt), L.ptr(out[PAD:]), old, L.ptr(cnt[PAD:]), old)
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.load().d3p_last_error())
    if expect != 0:
        assert bool((out == CANARY).all()) and bool((cnt == ICANARY).all()), "a refused call wrote"
        return None
    body, cbody = out[PAD:PAD + 4 * old].reshape(4, old), cnt[PAD:PAD + 2 * old].reshape(2, old)
    assert bool((out[:PAD] == CANARY).all()) and bool((out[PAD + 4 * old:] == CANARY).all()) and bool((body[:, cols:] == CANARY).all()), \
        "the scores were written outside their extent"
    assert bool((cnt[:PAD] == ICANARY).all()) and bool((cnt[PAD + 2 * old:] == ICANARY).all()) and bool((cbody[:, cols:] == ICANARY).all()), \
        "the counts were written outside their extent"
    assert np.array_equal(bits(np_(mat[:, :cols])), bits(m)) and bool((mat[:, cols:] == (ICANARY if is_int else CANARY)).all())
    return np_(body[:, :cols]).copy(), np_(cbody[:, :cols]).astype(np.int64)


def check(m, y, lds, what):
    """The entry at every ld of lds against score_at within bound, the counts by value: the largest error / bound seen."""
    want, want_counts = SR.score_at(m, y)
    tol = SR.bound(m, y, want)
    assert np.array_equal(np.isnan(want[0]), SR.nonfinite(m, y))
    worst = 0.0
    for ld in lds:
        got, got_counts = entry(m, y, ld)
        assert np.array_equal(got_counts, want_counts), f"{what} ld={ld}: the counts differ"
        ok, ratio = SR.within(got, want, tol)
        assert ok, f"{what} ld={ld}: error / bound = {ratio}"
        worst = max(worst, ratio)
    return worst


def sweep(n, col_set, kinds, lds=None):
    worst = 0.0
    for cols in col_set:
        for kind in kinds:
            m = SR.matrix(kind, n, cols)
            K = len(SR.y_kinds(m))
            for r in range(K if cols < K else 1):           # (fewer columns than kinds of y: every rotation, so that each kind is met)
                y = SR.observations(m, SR.rotation(m, r))
                worst = max(worst, check(m, y, lds or (cols, cols + 64), f"{kind} n={n} cols={cols} rotation {r}"))
    return worst


# ---------------------------------------------------------------- 1. the entry alone against the comparator
@pytest.mark.parametrize("n_spec", [1, 2, 3, 9, 31, 128, 257, 1025, "N32", "N32+1", "N8", "N8+1"])
def test_direct_entry_lies_within_the_bound_of_the_comparator(gpu, FORMS, n_spec):
    """Every kind of matrix crossed with every kind of y, at cols around the three forms' 32, 8 and 2 columns, ld = cols and cols + 64;
    n around the network's powers of two and on both sides of each form's limit."""
    n32, n8, _ = FORMS
    n = {"N32": n32, "N32+1": n32 + 1, "N8": n8, "N8+1": n8 + 1}.get(n_spec, n_spec)
    worst = sweep(n, (1, 2, 3, 33) if n >= n8 else (1, 7, 8, 9, 31, 32, 33, 300), SR.KINDS)
    print(f"\nd3p_col_crps n={n}: largest error / bound = {worst:.4f}")


def test_direct_entry_at_the_largest_n(gpu, FORMS):
    worst = sweep(FORMS[2], (1, 2, 3, 33), SR.KINDS)
    print(f"\nd3p_col_crps n={FORMS[2]}: largest error / bound = {worst:.4f}")


def test_fixed_columns_on_the_device(gpu):
    got, counts = entry(np.array([[4], [1], [2]], np.int32), np.array([3], np.int32))
    assert np.array_equal(got[:, 0], np.array([2 / 3, 1 / 3, 4 / 3, 2 / 3], np.float64).astype(np.float32)) and counts[:, 0].tolist() == [2, 0]
    got, counts = entry(np.array([[1.5, -2.0, 7.0]], np.float32), np.array([0.25, -2.0, 9.0], np.float32))     # n = 1
    assert np.array_equal(got[0], [1.25, 0.0, 2.0]) and np.isnan(got[1]).all() and np.array_equal(got[2], got[0]) and np.all(got[3] == 0.0)
    assert counts.tolist() == [[0, 0, 1], [0, 1, 0]]
    for n in (10, 257):                                                              # the Brier score of the draws' frequency
        m = SR.matrix("binary", n, 22)
        for yv in (0, 1):
            got, _ = entry(m, np.full(22, yv, np.int32))
            p = m.sum(axis=0).astype(np.float64) / n
            assert np.all(np.abs(got[0] - (p - yv) ** 2) <= SR.bound(m, np.full(22, yv, np.int32))[0])


@pytest.mark.parametrize("n_spec", [31, "N32+1", "N8+1"])
def test_a_non_finite_draw_or_observation_flags_its_column_and_no_other(gpu, FORMS, n_spec):
    n = {"N32+1": FORMS[0] + 1, "N8+1": FORMS[1] + 1}.get(n_spec, n_spec)
    m = SR.matrix("normal", n, 70)
    y = SR.observations(m, ["inside"] * 70)
    clean, clean_counts = entry(m, y)
    m2, y2 = m.copy(), y.copy()
    m2[n // 2, 33] = np.nan
    m2[0, 69] = -np.nan
    m2[3, 5], m2[4, 6] = -np.inf, np.inf
    y2[7], y2[8], y2[9] = np.nan, np.inf, -np.inf
    y2[33] = m[n // 2, 33]                                                           # (the draw the NaN replaced: it no longer counts as equal)
    got, counts = entry(m2, y2, 70 + 64)
    flagged = [5, 6, 7, 8, 9, 33, 69]
    keep = [c for c in range(70) if c not in flagged]
    assert np.isnan(got[:, flagged]).all() and not np.isnan(got[:, keep]).any()
    assert np.array_equal(bits(got[:, keep]), bits(clean[:, keep])) and np.array_equal(counts[:, keep], clean_counts[:, keep])
    want_counts = SR.counts(m2, y2)
    assert np.array_equal(counts, want_counts)                                       # IEEE counts, also on the flagged columns
    assert counts[:, 7].tolist() == [0, 0] and counts[:, 8].tolist() == [n, 0] and counts[:, 9].tolist() == [0, 0]
    assert counts[1, 33] == 0 and counts[:, 69].sum() <= n - 1


def test_negative_and_positive_zero_are_one_value(gpu):
    m = np.array([[-0.0, 0.0, 1.0], [0.0, -0.0, -0.0], [-0.0, -0.0, 0.0], [0.0, 0.0, -1.0]], np.float32)
    for y in (np.array([0.0, -0.0, 0.0], np.float32), np.array([-0.0, 0.0, -0.0], np.float32)):
        got, counts = entry(m, y)
        assert counts.tolist() == [[0, 0, 1], [4, 4, 2]] and np.all(got[:, :2] == 0.0)
        flipped, fcounts = entry(-m, y)
        assert np.array_equal(bits(flipped[:, :2]), bits(got[:, :2])) and fcounts[:, :2].tolist() == [[0, 0], [4, 4]]


# ---------------------------------------------------------------- 2. independence
@pytest.mark.parametrize("n_spec", [31, "N32+1", "N8+1"])
def test_a_columns_bits_depend_on_its_values_its_observation_and_n_alone(gpu, FORMS, n_spec):
    """Permuting the columns together with y permutes all six outputs bit for bit; permuting the draws within the columns changes no
    bit; a column alone gives the bits it gives among 300; neither ld nor a second call changes a bit."""
    n = {"N32+1": FORMS[0] + 1, "N8+1": FORMS[1] + 1}.get(n_spec, n_spec)
    cols = 300
    rng = np.random.default_rng(n)
    for kind in ("normal", "quarters", "counts", "lognormal"):
        m = SR.matrix(kind, n, cols)
        y = SR.observations(m, SR.rotation(m, 3))
        if m.dtype == np.float32:
            y[[k in ("nan", "plus_inf", "minus_inf") for k in SR.rotation(m, 3)]] = 0.25    # (finite everywhere: every bit is a number's)
        whole, counts = entry(m, y, cols + 64)
        assert not np.isnan(whole[[0, 2, 3]]).any()
        perm = rng.permutation(cols)
        moved, moved_counts = entry(np.ascontiguousarray(m[:, perm]), y[perm], cols)
        assert np.array_equal(bits(moved), bits(whole[:, perm])) and np.array_equal(moved_counts, counts[:, perm]), f"{kind}: a column's place"
        shuffled = np.stack([m[rng.permutation(n), c] for c in range(cols)], axis=1)
        mixed, mixed_counts = entry(shuffled, y, cols + 64)
        assert np.array_equal(bits(mixed), bits(whole)) and np.array_equal(mixed_counts, counts), f"{kind}: the order of the draws"
        for c in (0, 123, 299):
            alone, alone_counts = entry(np.ascontiguousarray(m[:, c:c + 1]), y[c:c + 1], 1)
            assert np.array_equal(bits(alone[:, 0]), bits(whole[:, c])) and np.array_equal(alone_counts[:, 0], counts[:, c]), f"{kind}: column {c} alone"
        again, _ = entry(m, y, cols)
        assert np.array_equal(bits(again), bits(whole)), f"{kind}: ld or a second call changes the bits"


# ---------------------------------------------------------------- 3. refusals
def test_more_draws_than_the_sort_holds_are_refused_and_nothing_is_written(gpu, FORMS):
    import d3p_amd._lib as L
    nmax = FORMS[2]
    m = np.zeros((nmax + 1, 3), np.float32)
    entry(m, np.zeros(3, np.float32), 3 + 64, expect=-3)                             # D3P_E_UNSUPPORTED: there is no streamed form
    assert str(nmax).encode() in L.load().d3p_last_error()
    entry(m.astype(np.int32), np.zeros(3, np.int32), expect=-3)


def test_col_crps_refuses_what_is_not_device_memory(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    n, cols = 9, 40
    mat, y = torch.zeros((n, cols), device="cuda"), torch.zeros(cols, device="cuda")
    out = torch.full((4, cols), CANARY, device="cuda")
    cnt = torch.full((2, cols), ICANARY, dtype=torch.int32, device="cuda")

    def run(mat_=L.ptr(mat), y_=L.ptr(y), out_=L.ptr(out), cnt_=L.ptr(cnt), cols_=cols):
        return lib.d3p_col_crps(L.stream_ptr(), mat_, 0, cols, n, cols_, y_, out_, cols, cnt_, cols)
    hosts = (torch.zeros((n, cols)), torch.zeros(cols), torch.zeros((4, cols)), torch.zeros((2, cols), dtype=torch.int32))
    for name, host in zip(("mat_", "y_", "out_", "cnt_"), hosts):
        assert run(**{name: L.ptr(host)}) == -1 and b"device memory" in lib.d3p_last_error()
    assert run(cols_=32 * (2 ** 31 - 1) + 1) == -1                                   # (ld < cols comes first)
    assert run(cols_=0) == 0
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((cnt == ICANARY).all())              # nothing was launched
    assert run() == 0
    torch.cuda.synchronize()
    assert bool((out[[0, 2, 3]] == 0.0).all()) and bool((cnt[0] == 0).all()) and bool((cnt[1] == n).all())


# ---------------------------------------------------------------- 4. the Python surface: score_draws, crps, pit
def test_score_draws_on_float32_int32_and_strided_views(SC, FORMS):
    for kind in ("lognormal", "counts", "binary"):
        m = SR.matrix(kind, 257, 70)
        y = SR.observations(m, ["inside", "one_draw", "tied_run", "above_all", "below_all"] * 14)
        t, yt = torch.tensor(m).cuda(), torch.tensor(y).cuda()
        s = SC.score_draws(t, yt)
        assert sorted(s) == ["below", "crps", "crps_fair", "equal", "mae", "spread"]
        assert all(s[k].shape == (70,) and s[k].is_cuda and s[k].dtype == (torch.int32 if k in ("below", "equal") else torch.float32) for k in s)
        raw, raw_counts = entry(m, y)
        for i, k in enumerate(SR.ROWS):
            assert np.array_equal(bits(np_(s[k])), bits(raw[i])), (kind, k)
        assert np.array_equal(np_(s["below"]), raw_counts[0]) and np.array_equal(np_(s["equal"]), raw_counts[1])
        assert torch.equal(SC.crps(t, yt), s["crps"]) and torch.equal(SC.crps(t, yt, fair=True), s["crps_fair"])
        lower, upper = SC.pit(t, yt)
        assert lower.dtype == torch.float32 and torch.equal(lower, s["below"].float() / 257) and torch.equal(upper, (s["below"] + s["equal"]).float() / 257)
        assert np.array_equal(np_(SC.score_draws(t, y)["crps"]), np_(s["crps"]))                      # a numpy y
        if m.dtype == np.int32:                                                       # a float y with integral values is cast
            assert torch.equal(SC.score_draws(t, yt.double())["crps"], s["crps"]) and torch.equal(SC.crps(t, y.astype(np.float64)), s["crps"])
            with pytest.raises(ValueError, match="non-integral"):
                SC.score_draws(t, yt.float() + 0.5)
        view, yv = t[::2, 3:40], yt[3:40]                                             # strided rows, offset columns
        assert view.stride(0) == 140 and not view.is_contiguous()
        want, want_counts = entry(np.ascontiguousarray(m[::2, 3:40]), y[3:40])
        got = SC.score_draws(view, yv)
        assert np.array_equal(bits(np_(got["crps"])), bits(want[0])) and np.array_equal(np_(got["equal"]), want_counts[1])
        one = SC.score_draws(t[:1], yt)
        assert bool(torch.isnan(one["crps_fair"]).all()) and torch.equal(one["crps"], one["mae"])
    empty = SC.score_draws(torch.zeros((5, 0), device="cuda"), torch.zeros(0))
    assert empty["crps"].shape == (0,) and empty["below"].shape == (0,)
    with pytest.raises(ValueError, match=rf"n <= {FORMS[2]}\b"):
        SC.score_draws(torch.zeros((FORMS[2] + 1, 2), device="cuda"), torch.zeros(2))
    with pytest.raises(ValueError, match="unit stride"):
        SC.score_draws(torch.zeros((4, 6), device="cuda")[:, ::2], torch.zeros(3))
    with pytest.raises(ValueError, match="3 observations expected"):
        SC.score_draws(torch.zeros((4, 3), device="cuda"), torch.zeros(4))


# ---------------------------------------------------------------- 5. the regression families
def make_model(family, d, intercept):
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    if family == "logistic":
        return LogisticRegression(d, intercept=intercept)
    if family == "linear":
        return LinearRegression(d, intercept=intercept, obs_scale=MR.SIGMA["linear"])
    return PoissonRegression(d, intercept=intercept)


def samples_of(W, b):
    return {"w": torch.tensor(np.array(W)).cuda(), "intercept": torch.tensor(np.array(b)).cuda()}


def _guide_params(model, d):
    from d3p_amd.models import AutoDiagonalNormal
    guide = AutoDiagonalNormal(model)
    params = {k: torch.tensor(v) for k, v in P.logreg_params(guide, d, True, np.random.default_rng(12)).items()}
    params["auto_loc"] = 0.2 * params["auto_loc"]                 # (keeps the Poisson rates moderate)
    return guide, params


def _assert_result(SC, res, obs, yt, n, rows, fair=False):
    """res equals score_draws on the sampled outcomes bit for bit, and its totals the float64 reductions of the pointwise arrays."""
    s = SC.score_draws(obs, yt)
    pw = res.pointwise
    assert sorted(pw) == ["crps", "mae", "pit_lower", "pit_upper", "spread"] and (res.n_draws, res.n_rows) == (n, rows)
    assert np.array_equal(bits(np_(pw["crps"])), bits(np_(s["crps_fair" if fair else "crps"])))
    assert np.array_equal(bits(np_(pw["mae"])), bits(np_(s["mae"]))) and np.array_equal(bits(np_(pw["spread"])), bits(np_(s["spread"])))
    lower, upper = SC.pit(obs, yt)
    assert torch.equal(pw["pit_lower"], lower) and torch.equal(pw["pit_upper"], upper)
    x = pw["crps"].double()
    assert res.crps.dtype == torch.float64 and res.crps.dim() == 0
    assert float(res.crps) == float(x.sum() / rows) and float(res.mae) == float(pw["mae"].double().sum() / rows)
    assert float(res.spread) == float(pw["spread"].double().sum() / rows)
    assert abs(float(res.crps) - float(x.mean())) <= 1e-14 * abs(float(x.mean()))
    assert abs(float(res.se) - float(x.std() / rows ** 0.5)) <= 1e-12 * float(res.se)
    assert torch.equal(res.pit_histogram, SC.pit_histogram(lower, upper, 10)) and abs(float(res.pit_histogram.sum()) - rows) < 1e-9


@pytest.mark.parametrize("family", MR.FAMILIES)
def test_predictive_crps_scores_the_sampled_outcomes(SC, family):
    from d3p_amd import predictive as PS
    n, rows, d = 100, 300, 4
    X, y, W, b = LR.inputs(family, n, rows, d, True, seed=61)
    model, Xt, s, key = make_model(family, d, True), torch.tensor(X).cuda(), samples_of(W, b), P.key(5)
    obs = PS.predictive_samples(key, model, s, Xt)
    assert obs.dtype == (torch.float32 if family == "linear" else torch.int32) and obs.shape == (n, rows)
    yt = torch.tensor(y).cuda().to(obs.dtype)
    res = SC.predictive_crps(key, model, s, Xt, torch.tensor(y).cuda(), rows, pointwise=True)
    _assert_result(SC, res, obs, yt, n, rows)
    fair = SC.predictive_crps(key, model, s, Xt, y, pointwise=True, fair=True)          # (a numpy y)
    _assert_result(SC, fair, obs, yt, n, rows, fair=True)
    assert bool((fair.pointwise["crps"] <= res.pointwise["crps"]).all())               # the fair spread is the larger one
    plain = SC.predictive_crps(key, model, s, Xt, y, bins=5)
    assert plain.pointwise is None and float(plain.crps) == float(res.crps) and plain.pit_histogram.shape == (5,)
    if family == "logistic":                                                            # the Brier score of the draws' frequency
        p = obs.double().mean(dim=0)
        assert torch.allclose(res.pointwise["crps"].double(), (p - yt.double()) ** 2, rtol=0, atol=1e-7)
    same = SC.compare_scores(res, res)
    assert float(same.crps_diff) == 0.0 and float(same.se_diff) == 0.0
    other = SC.predictive_crps(P.key(6), model, s, Xt, y, pointwise=True)
    diff = SC.compare_scores(res, other)
    assert abs(float(diff.crps_diff) - (float(res.crps) - float(other.crps))) <= 1e-12 and float(diff.se_diff) > 0.0
    with pytest.raises(ValueError, match=rf"slab_bytes >= {4 * n * rows}\b"):
        SC.predictive_crps(key, model, s, Xt, y, slab_bytes=4 * n * 128)


@pytest.mark.parametrize("family", MR.FAMILIES)
def test_posterior_predictive_crps_scores_the_posterior_draws(SC, family):
    from d3p_amd import predictive as PS
    n, rows, d = 100, 300, 4
    X, y, _, _ = LR.inputs(family, 1, rows, d, True, seed=41)
    model = make_model(family, d, True)
    guide, params = _guide_params(model, d)
    Xt, key = torch.tensor(X).cuda(), P.key(77)
    obs = PS.posterior_predictive_samples(key, n, model, (Xt,), guide, params)["obs"]
    res = SC.posterior_predictive_crps(key, n, model, (Xt, y), guide, params, pointwise=True)
    _assert_result(SC, res, obs.reshape(n, rows), torch.tensor(y).cuda().to(obs.dtype), n, rows)
    other = SC.posterior_predictive_crps(P.key(78), n, model, (Xt, y), guide, params, pointwise=True)
    assert not torch.equal(other.pointwise["crps"], res.pointwise["crps"])


# ---------------------------------------------------------------- 6. examples
def _example(name):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ex_crps_" + name, os.path.join(root, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["linear_regression", "poisson_regression"])
def test_examples_report_crps_and_the_pit_histogram(SC, capsys, name):
    mod = _example(name)
    base = dict(sigma=0.5, clip_threshold=1.0, num_steps=300, learning_rate=2e-2, batch_size=200, dimensions=4, num_samples=2000, obs_scale=0.5)
    mod.main(argparse.Namespace(crps=50, **base))
    out = capsys.readouterr().out
    m = re.search(r"^CRPS on the test split \(2000 rows, 50 draws\): ([\d.]+) \+- ([\d.]+)\nmae ([\d.]+), spread ([\d.]+)\n"
                  r"PIT histogram \(density, 10 bins\): ((?:[\d.]+ ?){10})$", out, re.M)
    assert m, out
    crps, se, mae, spread = (float(m.group(i)) for i in range(1, 5))
    assert 0.0 < crps < mae and se > 0.0 and abs(crps - (mae - spread)) <= 2e-4
    density = [float(v) for v in m.group(5).split()]
    assert len(density) == 10 and abs(sum(density) - 10.0) < 0.01 and all(v >= 0.0 for v in density)
    mod.main(argparse.Namespace(**base))
    assert "CRPS" not in capsys.readouterr().out
