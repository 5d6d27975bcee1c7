"""d3p_pair_knn and d3p_amd.neighbours on the GPU under each forced form: integer tables BY VALUE against tests/neighbours_ref.py (every q
is exact), float tables by property against tests/fidelity_ref.py, and what the contract calls independent bit for bit."""
import argparse
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import fidelity_ref as FR
from tests import neighbours_ref as NR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("sq", "distance", "index", "count")
_REF = {}      # case -> the comparator's outputs: computed once, shared by the forms, never changed


def bits(out, rows=slice(None)):
    return tuple(np.ascontiguousarray(out[k][rows]).tobytes() for k in KEYS if k in out)


@pytest.fixture(scope="module")
def LIB(gpu):
    import d3p_amd._lib as L
    return L.load()


@pytest.fixture(scope="module")
def TCS(LIB):      # rows a side of a pair tile, columns of a chunk, tiles of b per segment at the shapes used here, the largest k
    T = int(LIB.d3p_pair_knn_tile_rows())
    return T, int(LIB.d3p_pair_knn_chunk_cols()), int(LIB.d3p_pair_knn_segment_tiles(T + 1, T + 1, 3, 1)), int(LIB.d3p_pair_knn_max_k())


@pytest.fixture(params=(1, 2), ids=["wide-form", "split-form"])
def form(request, LIB):
    assert LIB.d3p_pair_knn_set_form(request.param) == 0
    yield request.param
    assert LIB.d3p_pair_knn_set_form(0) == 0


def _table(t, pad):
    buf = torch.full((t.shape[0] * (t.shape[1] + pad),), 12345, dtype=torch.int32 if t.dtype == np.int32 else torch.float32, device="cuda")
    buf.as_strided(t.shape, (t.shape[1] + pad, 1)).copy_(torch.tensor(t))
    return buf, t.shape[1] + pad


def entry(a, b, k, excl=False, radius=None, pads=(0, 0), ws_fill=0xFF):
    import d3p_amd._lib as L                    # (row strides d + pads; the outputs and the workspace hold 0xFF bytes on entry)
    lib, (na, d), nb = L.load(), a.shape, b.shape[0]
    (ab, a_ld), (bb, b_ld) = _table(a, pads[0]), _table(b, pads[1])
    rad = torch.tensor(radius, dtype=torch.float32, device="cuda") if radius is not None else None
    sq, dist, idx, cnt = (torch.full((na, w), -1, dtype=torch.int32, device="cuda") for w in (k, k, k, 1))
    need = int(lib.d3p_pair_knn_workspace(na, nb, d, k))
    ws = torch.full((need,), ws_fill, dtype=torch.uint8, device="cuda") if need else None
    rc = lib.d3p_pair_knn(L.stream_ptr(), L.ptr(ab), L.ptr(bb), int(a.dtype == np.int32), a_ld, b_ld, na, nb, d, k, int(excl), L.ptr(rad),
                          L.ptr(sq), L.ptr(dist), L.ptr(idx), L.ptr(cnt), L.ptr(ws), need)
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.d3p_last_error())
    out = {"sq": sq.view(torch.float32), "distance": dist.view(torch.float32), "index": idx.long(), "count": cnt[:, 0].long()}
    return {key: v.cpu().numpy() for key, v in out.items() if key != "count" or radius is not None}


def test_integer_tables_by_value(form, TCS):
    """Ties are frequent; integer radii with 0, +inf and NaN; rows of b duplicated across a tile edge and a segment edge; nb < k."""
    T, C, S, KMAX = TCS
    ns = (1, 2, T - 1, T, T + 1, S * T - 1, S * T, S * T + 1, 2 * S * T + 1)
    cases = [(n, T + 1, 3, 5, False) for n in ns] + [(T + 1, n, 3, 5, False) for n in ns]
    cases += [(T + 1, 2 * T + 1, d, 5, False) for d in (1, C - 1, C, C + 1, 2 * C + 1)]
    cases += [(T + 3, S * T + 5, 3, k, False) for k in (1, 2, 4, 8, 9, KMAX)]                       # each capacity class's edge and edge + 1
    cases += [(5, 3, 2, 5, False), (5, 5, 2, 5, True), (1, 1, 2, 2, True), (S * T + 1, S * T + 1, 2, 2, True)]
    for i, (na, nb, d, k, excl) in enumerate(cases):
        rng = np.random.default_rng(100 + i)
        a = rng.integers(-6, 7, (na, d)).astype(np.int32 if i % 2 else np.float32)
        b = a if excl else rng.integers(-6, 7, (nb, d)).astype(a.dtype)
        if nb > S * T:
            b[T - 1], b[S * T - 1] = b[T], b[S * T]
        u = rng.random(nb)
        rad = np.where(u < 0.1, np.inf, np.where(u > 0.9, np.nan, rng.integers(0, 30, nb))).astype(np.float32) if i % 3 else None
        if i not in _REF:
            _REF[i] = NR.knn(a, b, k, excl, rad)
        pad = ((0, 0), (1, 0), (0, 7), (5, 3))[i % 4]
        got = entry(a, b, k, excl, rad, (pad[0], pad[0]) if excl else pad)
        for key in got.keys() | _REF[i].keys():
            assert np.array_equal(got[key], _REF[i][key], equal_nan=True), (form, (na, nb, d, k, excl), key)


def test_k_1_equals_pair_stats_bit_for_bit(form, TCS):
    from d3p_amd import fidelity as F, neighbours as N
    (T, C, S, KMAX), rng = TCS, np.random.default_rng(11)
    a, b = (torch.tensor(rng.normal(size=(n, C + 3)).astype(np.float32)).cuda() for n in (T + 5, 2 * S * T + 9))
    for x, y, excl in ((a, b, False), (b, b, True)):
        ps, nn = F.pair_stats(x, y, excl), N.knn(x, y, 1, excl)
        assert torch.equal(nn["distance"][:, 0].view(torch.int32), ps["min"].view(torch.int32)) and torch.equal(nn["index"][:, 0], ps["argmin"])
    # a partial tile on each side, two column chunks and the diagonal, both entries in the same forced form
    c = torch.tensor(rng.normal(size=(T + 1, C + 1)).astype(np.float32)).cuda()
    import d3p_amd._lib as L
    try:
        assert L.load().d3p_pair_stats_set_form(form) == 0
        ps, nn = F.pair_stats(c, c, True), N.knn(c, c, 1, True)
    finally:
        assert L.load().d3p_pair_stats_set_form(0) == 0
    assert torch.equal(nn["distance"][:, 0].view(torch.int32), ps["min"].view(torch.int32)) and torch.equal(nn["index"][:, 0], ps["argmin"])


@pytest.mark.parametrize("name", ["normal", "d784", "far-cluster"])
def test_float_tables_by_property(form, TCS, name):
    T, C, S, KMAX = TCS
    rng = np.random.default_rng(12)
    a, b, excl = {"normal": lambda: (rng.normal(size=(T + 3, C + 3)), rng.normal(size=(2 * S * T + 9, C + 3)), False),
                  "d784": lambda: (rng.random(size=(T + 1, 784)), rng.random(size=(T + 1, 784)), False),
                  "far-cluster": lambda: (1.0e4 + 1.0e-3 * rng.normal(size=(S * T + 3, 2)), None, True)}[name]()    # (a Gram matrix loses these)
    a = a.astype(np.float32)
    b, k, (na, d) = a if excl else b.astype(np.float32), 5, a.shape
    if name not in _REF:
        dist = FR.exact(a, b, excl)["dist"]
        if excl:
            np.fill_diagonal(dist, np.inf)
        _REF[name] = (dist, np.sort(dist, axis=1)[:, :k])
    (dist, want), got, rows = _REF[name], entry(a, b, k, excl, pads=(3, 3)), np.arange(na)[:, None]
    assert (got["index"] >= 0).all() and (got["index"] < b.shape[0]).all() and not (excl and (got["index"] == rows).any())
    assert all(len(set(r)) == k for r in got["index"].tolist()) and (np.diff(got["sq"], axis=1) >= 0).all()
    rho = FR.rho(d)
    assert (dist[rows, got["index"]] <= want * (1.0 + 2.0 * rho)).all()              # the t-th returned row is as near as the exact t-th
    err, tol = np.abs(got["distance"].astype(np.float64) - want), rho * want + FR._half_ulp32(want + rho * want)
    assert (err <= tol).all() and got["distance"].tobytes() == np.sqrt(got["sq"]).astype(np.float32).tobytes(), float((err - tol).max())


def test_a_rows_bits_depend_on_that_row_and_b_alone(LIB, TCS):
    T, C, S, KMAX = TCS
    rng = np.random.default_rng(20)
    na, nb, d, k = 2 * T + 5, 2 * S * T + 9, C + 3, 5
    a, b = rng.normal(size=(na, d)).astype(np.float32), rng.normal(size=(nb, d)).astype(np.float32)
    rad, runs = np.full(nb, np.float32(1.5 * d)), {}
    for f in (1, 2):
        assert LIB.d3p_pair_knn_set_form(f) == 0
        base = runs[f] = entry(a, b, k, radius=rad)
        assert 0 < base["count"].mean() < nb                                                        # (the radii cut through the table)
        assert bits(entry(a, b, k, radius=rad)) == bits(base)                                        # a repeat call
        assert bits(entry(a, b, k, radius=rad, pads=(3, 11))) == bits(base)                          # other strides
        for fill in (0x00, 0x5A):
            assert bits(entry(a, b, k, radius=rad, ws_fill=fill)) == bits(base)                      # what the workspace held
        perm = rng.permutation(na)                                                                   # another place in the tile, other neighbours
        assert bits(entry(a[perm], b, k, radius=rad), np.argsort(perm)) == bits(base)
        for lo, keep in ((5, 1), (T - 3, 7), (0, T + 1)):                                            # another na
            assert bits(entry(a[lo:lo + keep], b, k, radius=rad)) == bits(base, slice(lo, lo + keep))
    assert LIB.d3p_pair_knn_set_form(0) == 0
    assert bits(runs[1]) == bits(runs[2]) == bits(entry(a, b, k, radius=rad))                        # the forms agree, and so does the rule's choice


def test_flagged_rows_leave_their_neighbours_alone(form, TCS):
    T, C, S, KMAX = TCS
    rng = np.random.default_rng(40)
    na, nb, d, k = 2 * T + 1, S * T + 5, 3, 4
    a, b = rng.normal(size=(na, d)).astype(np.float32), rng.normal(size=(nb, d)).astype(np.float32)
    rad, bad, special = np.ones(nb, np.float32), a.copy(), [1, T, 2 * T]
    base = entry(a, b, k, radius=rad)
    bad[1, 2], bad[T, 0], bad[2 * T, 1] = np.nan, np.inf, -np.inf                                    # (the last alone in its tile)
    got = entry(bad, b, k, radius=rad)
    keep = [r for r in range(na) if r not in special]
    assert bits(got, keep) == bits(base, keep)
    assert np.isnan(got["sq"][special]).all() and np.isnan(got["distance"][special]).all()
    assert (got["index"][special] == -1).all() and (got["count"][special] == -1).all()
    for where in (3, S * T + 2):                                                                     # in b, first and last segment: every row
        bad_b = b.copy()
        bad_b[where, 1] = np.nan
        got = entry(a, bad_b, k, radius=rad)
        assert np.isnan(got["sq"]).all() and np.isnan(got["distance"]).all() and (got["index"] == -1).all() and (got["count"] == -1).all()


def test_prdc_against_the_restatement(form, TCS):
    from d3p_amd import neighbours as N
    (T, C, S, KMAX), rng = TCS, np.random.default_rng(70)
    real, synth, hold = (rng.integers(-6, 7, (n, 3)).astype(np.float32) for n in (S * T + 9, S * T - 5, 2 * T + 3))
    synth[:4] = real[10:14]                                              # four copied records
    rt, st, ht = (torch.tensor(v).cuda() for v in (real, synth, hold))
    got, want = N.prdc(rt, st, k=5, holdout=ht), NR.prdc(real, synth, 5, hold)
    numbers = ("precision", "recall", "density", "coverage", "authenticity")
    assert (got.k, got.n_real, got.n_synthetic, got.dim, got.floor.n_synthetic, got.floor.floor) == (5, S * T + 9, S * T - 5, 3, 2 * T + 3, None)
    assert [getattr(got, key) for key in numbers] == [want[key] for key in numbers] and got.authenticity < 1.0
    assert [getattr(got.floor, key) for key in numbers] == [want["floor"][key] for key in numbers]
    assert N.prdc(rt.to(torch.int32), st.to(torch.int32), k=5)[:5] == got[:5] and N.prdc(rt, st).floor is None
    x = torch.tensor(rng.normal(size=(S * T + 3, 4)).astype(np.float32)).cuda()
    same, away = N.prdc(x, x.clone(), k=3), N.prdc(x, x + 100.0, k=3)
    assert same.precision == same.recall == same.coverage == 1.0 and same.authenticity == 0.0
    assert away.precision == away.recall == away.coverage == away.density == 0.0 and away.authenticity == 1.0
    two = torch.cat([x[:200], x[200:400] + 50.0])                        # two well-separated clusters; the synthetic table knows one
    part = N.prdc(two, x[:200:2] + 1.0e-3, k=3)                          # (beside rows of the first cluster: inside their balls)
    assert part.precision == 1.0 and part.recall < 0.6 and part.coverage < 0.6
    with pytest.raises(ValueError, match="NaN or infinite"):             # flagged rows have no count to average
        N.prdc(x, torch.cat([x[:9], x[:1] * float("nan")]), k=3)
    kth, nn = N.kth_neighbour(x, 3), N.knn(x, x, 3, exclude_diagonal=True)
    assert torch.equal(kth["sq"], nn["sq"][:, 2]) and torch.equal(kth["distance"], nn["distance"][:, 2])
    assert torch.equal(N.ball_counts(x, two, kth["sq"][:400]), N.knn(x, two, 1, radius_sq=kth["sq"][:400])["count"])


def test_example_flag_reports_the_prdc_line(form, capsys):
    spec = importlib.util.spec_from_file_location("ex_gmm_prdc", os.path.join(ROOT, "examples", "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["--prdc"]).prdc == 5 and mod.parse_args(["--prdc", "3"]).prdc == 3 and mod.parse_args([]).prdc is None
    mod.main(argparse.Namespace(num_epochs=2, learning_rate=5e-2, batch_size=64, dimensions=2, num_samples=512, num_components=3, sigma=0.3, prdc=5))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("k-NN balls")]
    m = re.fullmatch(r"k-NN balls \(k = 5, 512 synthetic rows\): precision ([0-9.]+), recall ([0-9.]+), density ([0-9.]+), coverage ([0-9.]+), "
                     r"authenticity ([0-9.]+); held-out floor \(512 rows\): ([0-9.]+), ([0-9.]+), ([0-9.]+), ([0-9.]+), ([0-9.]+)", lines[0])
    assert len(lines) == 1 and m
    for i in range(1, 11):
        assert float(m.group(i)) >= 0 and (i % 5 == 3 or float(m.group(i)) <= 1)          # (density is not bounded by 1)
