"""Pair statistics and the fidelity report on the GPU (d3p_pair_stats, d3p_amd.fidelity) against tests/fidelity_ref.py, every shape under
each forced form.  `sum` and `min` lie within the DERIVED bound of the float64 comparator (fidelity_ref.bound), NaN by class on exactly
the flagged rows, and the returned index is checked by property (the exact distance there is within 2 rho of the exact minimum); the
cases with exact arithmetic are compared BY VALUE, the first-index tie rule included, with duplicated rows of b on both sides of a tile
edge and of a segment edge; everything the contract calls independent -- the form, a repeat, the row's place, its neighbours, na, the
strides, what the workspace held -- is compared bit for bit.  Outputs and workspace are filled with 0xFF bytes before every call.  The
largest error-to-bound ratio is printed (pytest -s) and recorded in docs/experiments_fidelity.md."""
import argparse
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import fidelity_ref as FR
from tests import workspace_harness as WH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 12345.0
ICANARY = 12345
PAD = 64
FORMS = (1, 2)
_REF = {}      # case name -> (exact, bound): computed once, shared by the forms, never changed


def np_(t):
    return t.detach().cpu().numpy()


def bits(out):
    """The three outputs as one byte string per array: NaN equals NaN, -0.0 differs from 0.0."""
    return tuple(np.ascontiguousarray(out[k]).tobytes() for k in ("sum", "min", "argmin"))


def rows_of(out, idx):
    return {k: out[k][idx] for k in ("sum", "min", "argmin")}


@pytest.fixture(scope="module")
def LIB(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    yield lib
    assert lib.d3p_pair_stats_set_form(0) == 0


@pytest.fixture(scope="module")
def TCG(LIB):
    """(T, C, G) from the query functions: rows a side of a pair tile, columns of a staged chunk, tiles of b per segment."""
    return int(LIB.d3p_pair_stats_tile_rows()), int(LIB.d3p_pair_stats_chunk_cols()), int(LIB.d3p_pair_stats_segment_tiles())


@pytest.fixture(params=FORMS, ids=["wide-form", "split-form"])
def form(request, LIB):
    assert LIB.d3p_pair_stats_set_form(request.param) == 0
    yield request.param
    assert LIB.d3p_pair_stats_set_form(0) == 0


def _table(t, pad, tdt, can):
    n, d = t.shape
    ld = d + pad
    buf = torch.full((n * ld + PAD,), can, dtype=tdt, device="cuda")
    buf.as_strided((n, d), (ld, 1)).copy_(torch.tensor(t))
    return buf, ld


def entry(a, b, excl=False, pads=(0, 0), ws_fill=0xFF):
    """d3p_pair_stats on the numpy tables a (na, d) and b (nb, d) with a_ld = d + pads[0], b_ld = d + pads[1]; canaries in every padding,
    the outputs and the workspace pre-filled with 0xFF bytes between guards: {"sum", "min", "argmin" (int64, -1: none)} after the
    tables, the guards and the paddings were checked."""
    import d3p_amd._lib as L
    lib = L.load()
    a, b = (t[:, None] if t.ndim == 1 else t for t in (a, b))
    (na, d), nb = a.shape, b.shape[0]
    is_int = a.dtype == np.int32
    tdt, can = (torch.int32, ICANARY) if is_int else (torch.float32, CANARY)
    ab, a_ld = _table(a, pads[0], tdt, can)
    bb = ab if b is a and pads[0] == pads[1] else None          # (a table against itself: the same memory)
    if bb is None:
        bb, b_ld = _table(b, pads[1], tdt, can)
    else:
        b_ld = a_ld
    before = (ab.clone(), bb.clone())
    outs = [torch.full((PAD + na * w + PAD,), -1, dtype=torch.int32, device="cuda") for w in (2, 1, 1)]       # 0xFF bytes
    need = int(lib.d3p_pair_stats_workspace(na, nb, d))
    ws = torch.full((PAD * 4 + need + PAD * 4,), ws_fill, dtype=torch.uint8, device="cuda")
    rc = lib.d3p_pair_stats(L.stream_ptr(), L.ptr(ab), L.ptr(bb), int(is_int), a_ld, b_ld, na, nb, d, int(excl),
                            L.ptr(outs[0][PAD:]), L.ptr(outs[1][PAD:]), L.ptr(outs[2][PAD:]), L.ptr(ws[PAD * 4:]) if need else None, need)
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.d3p_last_error())
    assert torch.equal(ab.view(torch.int32), before[0].view(torch.int32)) and torch.equal(bb.view(torch.int32), before[1].view(torch.int32)), \
        "a table was written"
    for o, w in zip(outs, (2, 1, 1)):
        assert bool((o[:PAD] == -1).all()) and bool((o[PAD + na * w:] == -1).all()), "an output was written outside its extent"
    assert bool((ws[:PAD * 4] == ws_fill).all()) and bool((ws[PAD * 4 + need:] == ws_fill).all()), "the workspace was written outside its extent"
    idx = np_(outs[2][PAD:PAD + na]).astype(np.int64) & 0xFFFFFFFF
    return {"sum": np_(outs[0][PAD:PAD + 2 * na].contiguous().view(torch.float64)).copy(),
            "min": np_(outs[1][PAD:PAD + na].contiguous().view(torch.float32)).copy(), "argmin": np.where(idx == 0xFFFFFFFF, -1, idx)}


def data(seed, n, d, is_int):
    rng = np.random.default_rng(seed)
    return rng.integers(-50, 51, (n, d)).astype(np.int32) if is_int else rng.normal(size=(n, d)).astype(np.float32)


def reference(name, a, b, excl):
    if name not in _REF:
        ex = FR.exact(a, b, excl)
        _REF[name] = (ex, FR.bound(ex, b.shape[0], a.shape[1]))
    return _REF[name]


def within(got, ex, tol, d, excl):
    """got within tol of ex, NaN by class on exactly ex's NaNs, the index by property: the largest error / bound."""
    worst = 0.0
    for k in ("sum", "min"):
        nan = np.isnan(ex[k])
        assert np.array_equal(np.isnan(got[k]), nan), (k, got[k], ex[k])
        fin = ~nan & np.isfinite(ex[k])
        assert np.array_equal(got[k][~nan & ~fin], ex[k][~nan & ~fin]), k                      # (+inf where there is no pair)
        err = np.abs(got[k].astype(np.float64) - ex[k])[fin]
        assert (err <= tol[k][fin]).all(), (k, float((err / tol[k][fin]).max()))
        pos = tol[k][fin] > 0
        if pos.any():
            worst = max(worst, float((err[pos] / tol[k][fin][pos]).max()))
    none = ex["argmin"] < 0
    assert np.array_equal(got["argmin"] < 0, none)
    rows = np.nonzero(~none)[0]
    j = got["argmin"][rows]
    assert (j >= 0).all() and (j < ex["dist"].shape[1]).all() and not (excl and (j == rows).any())
    assert (ex["dist"][rows, j] <= ex["min"][rows] * (1.0 + 2.0 * FR.rho(d))).all()
    return worst


# ------------------------------------------------------------------------------------------------ against the comparator
def _sweep(T, C, G):
    ns = (1, 2, T - 1, T, T + 1, 2 * T + 1, G * T - 1, G * T, G * T + 1, 2 * G * T + 1)
    ds = (1, 2, 3, C - 1, C, C + 1, 2 * C + 1)
    cases = [(n, T + 1, 3, False) for n in ns] + [(T + 1, n, 3, False) for n in ns] + [(T + 1, 2 * T + 1, d, False) for d in ds]
    cases += [(n, n, 2, True) for n in ns]
    cases += [(2 * G * T + 1, 2 * G * T + 1, C + 1, False), (G * T + 1, G * T - 1, 2 * C + 1, False), (2, 2 * G * T + 1, C, False), (1, 1, 1, False),
              (G * T, G * T, 1, True), (2 * T + 1, G * T + 1, C - 1, False), (G * T - 1, 2, 2 * C + 1, False), (T, T, C, True)]
    return list(dict.fromkeys(cases))


def test_sweep_against_the_comparator_within_the_bound(form, TCG):
    T, C, G = TCG
    worst = 0.0
    for i, (na, nb, d, excl) in enumerate(_sweep(T, C, G)):
        is_int = i % 2 == 1
        a = data(100 + i, na, d, is_int)
        b = a if excl else data(500 + i, nb, d, is_int)
        ex, tol = reference(f"sweep{i}", a, b, excl)
        pads = ((0, 0), (1, 0), (0, 7), (5, 3))[i % 4]
        worst = max(worst, within(entry(a, b, excl, (pads[0], pads[0]) if excl else pads), ex, tol, d, excl))
    print(f"form {form}: largest error / bound over the sweep {worst:.4f}")


def test_the_vae_width_runs(form, TCG):
    T = TCG[0]
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 2, (T + 1, 784)).astype(np.int32), rng.integers(0, 2, (T + 1, 784)).astype(np.int32)
    ex, tol = reference("vae", a, b, False)
    print(f"form {form}: d = 784 error / bound {within(entry(a, b, pads=(16, 0)), ex, tol, 784, False):.4f}")


def test_clustered_far_from_the_origin(form, TCG):
    T, C, G = TCG
    rng = np.random.default_rng(8)
    a = (1.0e4 + 1.0e-3 * rng.normal(size=(G * T + 3, 2))).astype(np.float32)
    ex, tol = reference("far", a, a, True)
    print(f"form {form}: clustered rows error / bound {within(entry(a, a, True), ex, tol, 2, True):.4f}")


# ------------------------------------------------------------------------------------------------ by value
def _by_value(a, b, q, excl=False, pads=(1, 3)):
    """a, b with exact arithmetic: q the exact integer squared distances, every one a perfect square or compared through its rounded
    root -- sum, min and the FIRST index of the smallest q by value."""
    got = entry(a, b, excl, pads)
    q = q.astype(np.float64)
    if excl:
        q = q.copy()
        np.fill_diagonal(q, np.inf)
    root = np.sqrt(q.astype(np.float32)).astype(np.float32)            # (q < 2^24: exact in float32; the root correctly rounded)
    dist = np.where(np.isfinite(q), root.astype(np.float64), 0.0)
    want_sum = np.array([FR._fsum(r) for r in dist])
    assert np.array_equal(got["argmin"], np.argmin(q, axis=1)), "the first index of the smallest q"
    assert np.array_equal(got["min"], root[np.arange(q.shape[0]), np.argmin(q, axis=1)])
    return got, want_sum


def test_exact_cases_by_value(form, TCG):
    T, C, G = TCG
    rng = np.random.default_rng(9)
    # d = 1, small integers, both dtypes: every distance an integer, every float64 sum exact in any order
    for na, nb, dtype in ((3, 5, np.int32), (T + 3, 2 * G * T + 1, np.float32), (G * T + 1, T + 1, np.int32)):
        ka, kb = rng.integers(-20, 21, na), rng.integers(-20, 21, nb)
        got, want = _by_value(ka.astype(dtype), kb.astype(dtype), (ka[:, None] - kb[None, :]) ** 2)
        assert np.array_equal(got["sum"], want) and np.array_equal(want, np.abs(ka[:, None] - kb[None, :]).sum(axis=1))
    # d = 2, points k (3, 4): every distance is 5 |k_i - k_j|; a table against itself, the diagonal left out
    k = rng.integers(-30, 31, G * T + 2)
    z = (k[:, None] * np.array([3, 4])).astype(np.float32)
    got, want = _by_value(z, z, 25 * (k[:, None] - k[None, :]) ** 2, excl=True, pads=(2, 2))
    assert np.array_equal(got["sum"], want) and np.array_equal(want, 5.0 * np.abs(k[:, None] - k[None, :]).sum(axis=1))
    # every q = x^2 + y^2, 0 <= x, y <= 40, against the origin alone: the correctly rounded root of 1681 values, most no perfect square
    grid = np.stack(np.meshgrid(np.arange(41), np.arange(41)), axis=-1).reshape(-1, 2).astype(np.int32)
    got = entry(grid, np.zeros((1, 2), np.int32))
    root = np.sqrt((grid.astype(np.int64) ** 2).sum(axis=1).astype(np.float32)).astype(np.float32)
    assert np.array_equal(got["min"], root) and np.array_equal(got["sum"], root.astype(np.float64)) and (got["argmin"] == 0).all()
    # many ties: integer points of a small grid at d = 3, q an integer; the sums hold roots, so they are compared within the bound
    a, b = rng.integers(-3, 4, (2 * T + 1, 3)).astype(np.int32), rng.integers(-3, 4, (2 * G * T + 1, 3)).astype(np.int32)
    q = ((a[:, None, :].astype(np.int64) - b[None, :, :]) ** 2).sum(axis=2)
    got, want = _by_value(a, b, q)
    assert (np.abs(got["sum"] - want) <= (b.shape[0] + 16) * 2.0 ** -53 * want).all()
    # duplicated rows of b on both sides of a tile edge (T - 1, T) and of a segment edge (G T - 1, G T), and in two segments (5, G T + 7)
    nb = G * T + T
    b = np.stack([100 + np.arange(nb), 100 + (7 * np.arange(nb)) % 50], axis=1).astype(np.int32)      # distinct rows, q < 2^24
    p = np.array([[7, 7], [9, -4], [-6, 2]], np.int32)
    b[T - 1] = b[T] = p[0]
    b[G * T - 1] = b[G * T] = p[1]
    b[5] = b[G * T + 7] = p[2]
    a = np.concatenate([p, p + 1, b[:T + 1]]).astype(np.int32)          # the points, near misses (equidistant from both copies), rows of b
    q = ((a[:, None, :].astype(np.int64) - b[None, :, :]) ** 2).sum(axis=2)
    got, _ = _by_value(a, b, q)
    assert got["argmin"][:6].tolist() == [T - 1, G * T - 1, 5] * 2 and got["min"][:3].tolist() == [0.0] * 3
    assert (got["min"][3:6] == np.float32(np.sqrt(np.float32(2.0)))).all()
    # the same table against itself: a duplicate is a pair like any other (min = 0 at the OTHER copy), only j == i is skipped
    q = ((b[:, None, :].astype(np.int64) - b[None, :, :]) ** 2).sum(axis=2)
    got, _ = _by_value(b, b, q, excl=True, pads=(0, 0))
    for lo, hi in ((T - 1, T), (G * T - 1, G * T), (5, G * T + 7)):
        assert got["min"][lo] == 0.0 and got["min"][hi] == 0.0 and got["argmin"][lo] == hi and got["argmin"][hi] == lo
    assert (got["min"] == 0.0).sum() == 6
    # one row against itself without the diagonal: no admissible pair
    got = entry(a[:1], a[:1], True)
    assert got["sum"][0] == 0.0 and not np.signbit(got["sum"][0]) and got["min"][0] == np.inf and got["argmin"][0] == -1


# ------------------------------------------------------------------------------------------------ determinism
def test_a_rows_bits_depend_on_that_row_and_b_alone(LIB, TCG):
    T, C, G = TCG
    na, nb, d = 2 * T + 5, 2 * G * T + 9, C + 3
    a, b = data(20, na, d, False), data(21, nb, d, False)
    runs = {}
    for f in FORMS:
        assert LIB.d3p_pair_stats_set_form(f) == 0
        base = entry(a, b)
        assert bits(entry(a, b)) == bits(base)                                                       # a repeat call
        assert bits(entry(a, b, pads=(3, 11))) == bits(base)                                         # other strides
        for fill in (0x00, 0x5A):
            assert bits(entry(a, b, ws_fill=fill)) == bits(base)                                     # what the workspace held
        perm = np.random.default_rng(22).permutation(na)                                             # another place in the tile, other neighbours
        assert bits(rows_of(entry(a[perm], b), np.argsort(perm))) == bits(base)
        other = data(23, na, d, False)
        other[7], other[T + 1] = a[7], a[T + 1]
        assert bits(rows_of(entry(other, b), [7, T + 1])) == bits(rows_of(base, [7, T + 1]))          # changed neighbours
        for lo, keep in ((5, 1), (T - 3, 7), (0, T + 1)):                                            # another na
            assert bits(entry(a[lo:lo + keep], b)) == bits(rows_of(base, slice(lo, lo + keep)))
        runs[f] = base
    assert LIB.d3p_pair_stats_set_form(0) == 0
    assert bits(runs[1]) == bits(runs[2])                                                            # the forms agree bit for bit
    assert bits(entry(a, b)) == bits(runs[1])                                                        # and so does the rule's choice
    x = data(24, G * T + 7, 2, False)                                                                # a table against itself
    runs = {}
    for f in FORMS:
        assert LIB.d3p_pair_stats_set_form(f) == 0
        runs[f] = entry(x, x, True)
        assert bits(entry(x, x, True, pads=(2, 2))) == bits(runs[f])
    assert LIB.d3p_pair_stats_set_form(0) == 0
    assert bits(runs[1]) == bits(runs[2])


@pytest.mark.parametrize("fill", ["zero", "ones", "bits"])
def test_workspace_contents_and_extent_through_the_python_layer(LIB, TCG, monkeypatch, fill):
    """The public function on guarded memory (tests/workspace_harness.py): no byte outside the workspace or the outputs is written,
    the pre-filled workspace changes no bit, and a workspace one byte short is refused with everything untouched."""
    import d3p_amd._lib as L
    from d3p_amd import fidelity as F
    T, C, G = TCG
    a, b = data(30, T + 3, 5, False), data(31, G * T + 4, 5, False)
    at, bt = torch.tensor(a).cuda(), torch.tensor(b).cuda()
    try:
        assert LIB.d3p_pair_stats_set_form(1) == 0
        want = F.pair_stats(at, bt)
        assert LIB.d3p_pair_stats_set_form(2) == 0
        need = int(LIB.d3p_pair_stats_workspace(T + 3, G * T + 4, 5))
        assert need == 2 * (T + 3) * 20
        rec = WH.Recorder(fill, 0, None)
        WH.guarded_empty(monkeypatch, F, rec, "pair_stats")
        got = F.pair_stats(at, bt)
        torch.cuda.synchronize()
        rec.check_all("pair_stats")
        assert [g.nbytes for g in rec.workspaces] == [need] and len(rec.buffers) == 4
        for k in ("sum", "min", "argmin"):
            assert torch.equal(WH.raw_bytes(got[k]), WH.raw_bytes(want[k])), (fill, k)
        short = WH.Recorder(fill, 1, None)
        WH.guarded_empty(monkeypatch, F, short, "pair_stats")
        with pytest.raises(L.D3PError, match="workspace too small"):
            F.pair_stats(at, bt)
        torch.cuda.synchronize()
        short.check_all("short")
        assert [g.nbytes for g in short.workspaces] == [need - 1]
        for g in short.buffers:                                        # outputs and workspace as they were handed out
            assert torch.equal(g.interior.cpu(), WH._fill_bytes(g.nbytes, g.fill, seed=g.seed)), g.tag
    finally:
        assert LIB.d3p_pair_stats_set_form(0) == 0


def test_special_rows_leave_their_neighbours_alone(form, TCG):
    T, C, G = TCG
    na, nb, d = 2 * T + 1, G * T + 5, 3
    a, b = data(40, na, d, False), data(41, nb, d, False)
    base = entry(a, b)
    bad = a.copy()
    bad[1, 2] = np.nan
    bad[T, 0] = np.inf
    bad[2 * T, 1] = -np.inf                          # (alone in the last tile of a)
    bad[7, :] = (1e30, 0.0, 0.0)                     # finite, but q overflows float32 against every row of b
    got = entry(bad, b)
    special = [1, T, 2 * T, 7]
    keep = [r for r in range(na) if r not in special]
    assert bits(rows_of(got, keep)) == bits(rows_of(base, keep))
    assert np.isnan(got["sum"][[1, T, 2 * T]]).all() and np.isnan(got["min"][[1, T, 2 * T]]).all() and (got["argmin"][[1, T, 2 * T]] == -1).all()
    assert got["sum"][7] == np.inf and got["min"][7] == np.inf and got["argmin"][7] == 0            # IEEE; ties at inf: the smallest j
    for where in (3, G * T + 2):                     # a NaN in b, in the first and in the last segment: every row
        bad_b = b.copy()
        bad_b[where, 1] = np.nan
        got = entry(a, bad_b)
        assert np.isnan(got["sum"]).all() and np.isnan(got["min"]).all() and (got["argmin"] == -1).all()
    far_b = b.copy()
    far_b[G * T + 1, 0] = -1e30                      # a finite row of b whose q overflows: the sums are inf, the nearest rows stay
    got = entry(a, far_b)
    kept = base["argmin"] != G * T + 1             # (the rows whose nearest row was not the one moved away)
    assert (got["sum"] == np.inf).all() and kept.sum() >= na - 2
    assert got["min"][kept].tobytes() == base["min"][kept].tobytes() and np.array_equal(got["argmin"][kept], base["argmin"][kept])
    one = entry(a[:1], a[:1], True)                  # nb = 1 with the diagonal excluded
    assert one["sum"][0] == 0.0 and one["min"][0] == np.inf and one["argmin"][0] == -1


# ------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer_on_the_device(gpu, TCG):
    from d3p_amd import fidelity as F
    T, C, G = TCG
    a, b = data(50, T + 2, 4, True), data(51, G * T + 3, 4, True)
    at, bt = torch.tensor(a).cuda(), torch.tensor(b).cuda()
    want = entry(a, b)
    got = F.pair_stats(at, bt)
    assert got["sum"].dtype == torch.float64 and got["min"].dtype == torch.float32 and got["argmin"].dtype == torch.int64
    assert all(got[k].shape == (T + 2,) for k in got) and bits({k: np_(v) for k, v in got.items()}) == bits(want)
    wide = torch.zeros((T + 2, 9), dtype=torch.int32, device="cuda")
    wide[:, :4] = at
    assert bits({k: np_(v) for k, v in F.pair_stats(wide[:, :4], bt).items()}) == bits(want)         # a strided view
    dcr = F.closest_record(at, bt)
    assert np.array_equal(np_(dcr["distance"]), want["min"]) and np.array_equal(np_(dcr["index"]), want["argmin"])
    one = F.pair_stats(at[:, 0], bt[:, 0])                                                           # the 1-D form: d = 1
    assert bits({k: np_(v) for k, v in one.items()}) == bits(entry(a[:, :1], b[:, :1]))
    alone = F.pair_stats(at[:1], at[:1], exclude_diagonal=True)
    assert float(alone["sum"][0]) == 0.0 and float(alone["min"][0]) == np.inf and int(alone["argmin"][0]) == -1
    for v in (2 ** 24 + 1, -2 ** 24 - 1):
        big = bt.clone()
        big[2, 1] = v
        with pytest.raises(ValueError, match="beyond 2\\^24"):
            F.pair_stats(at, big)
    edge = bt.clone()
    edge[2, 1] = 2 ** 24
    assert bool(torch.isfinite(F.pair_stats(at, edge)["sum"]).all())


def test_energy_distance_on_the_device(gpu, TCG):
    from d3p_amd import fidelity as F
    T, C, G = TCG
    x = torch.tensor(data(60, G * T + 3, 5, False)).cuda()
    same = F.energy_distance(x, x.clone())
    assert float(same.d2) == 0.0 and float(same.exy) == float(same.exx) == float(same.eyy) > 0 and float(same.d2_unbiased) < 0
    assert (same.n_x, same.n_y, same.dim) == (G * T + 3, G * T + 3, 5) and same.d2.dtype == torch.float64 and same.d2.dim() == 0
    rng = np.random.default_rng(61)
    xs, ys = rng.integers(-40, 41, 2 * T + 1), rng.integers(-10, 71, G * T + 1)
    num, den, (sxy, sxx, syy) = FR.closed_form_d1(xs, ys)
    nx, ny = len(xs), len(ys)
    for dtype in (torch.int32, torch.float32):
        ed = F.energy_distance(torch.tensor(xs, dtype=dtype).cuda(), torch.tensor(ys, dtype=dtype).cuda())
        assert float(ed.exy) == sxy / (nx * ny) and float(ed.exx) == sxx / (nx * nx) and float(ed.eyy) == syy / (ny * ny)   # exact sums
        assert float(ed.d2) == pytest.approx(num / den, rel=1e-13) and float(ed.d2) > 0
        assert float(ed.d2_unbiased) == pytest.approx(2 * sxy / (nx * ny) - sxx / (nx * (nx - 1)) - syy / (ny * (ny - 1)), rel=1e-13)
    lone = F.energy_distance(x[:1], x[1:4])
    assert np.isnan(float(lone.d2_unbiased)) and np.isfinite(float(lone.d2)) and float(lone.exx) == 0.0
    y = torch.tensor(data(62, T + 5, 5, False) + np.float32(0.5)).cuda()
    ed = F.energy_distance(x, y)
    xn, yn = np_(x), np_(y)
    ref = FR.energy(FR.exact(xn, yn)["sum"], FR.exact(xn, xn, True)["sum"], FR.exact(yn, yn, True)["sum"], xn.shape[0], yn.shape[0])
    scale = 2 * ref[2] + ref[3] + ref[4]
    assert abs(float(ed.d2) - ref[0]) <= 2 * FR.rho(5) * scale and abs(float(ed.d2_unbiased) - ref[1]) <= 2 * FR.rho(5) * scale
    assert float(ed.d2) > 0


def test_fidelity_report_against_the_restatement(gpu, TCG):
    """Integer tables: every q is exact in float32, so the device's minima ARE the emulation's and the counts and shares are compared by
    value; ties (which the small grid makes frequent) exercise the strict comparisons and the 1/2 of closer_to_train."""
    from d3p_amd import fidelity as F
    T, C, G = TCG
    rng = np.random.default_rng(70)
    train, synth, hold = (rng.integers(-6, 7, (n, 3)).astype(np.float32) for n in (G * T + 9, G * T - 5, 2 * T + 3))
    synth[:4] = train[10:14]                                             # four copied records
    probs = (0.05, 0.5, 0.95)
    tt, st, ht = (torch.tensor(v).cuda() for v in (train, synth, hold))
    rep = F.fidelity_report(tt, st, holdout=ht, probs=probs)
    ref = FR.report(train, synth, hold, probs)
    assert (rep.n_train, rep.n_synthetic, rep.n_holdout, rep.dim) == (G * T + 9, G * T - 5, 2 * T + 3, 3) and rep.dcr_probs == probs
    assert rep.n_exact_copies == ref["n_exact_copies"] >= 4
    for k in ("aa_truth", "aa_synth", "aa", "aa_holdout", "privacy_loss", "closer_to_train"):
        assert getattr(rep, k) == ref[k], (k, getattr(rep, k), ref[k])
    assert 0.0 < rep.closer_to_train < 1.0 and rep.dcr_quantiles == ref["dcr_quantiles"]
    for got, want in ((rep.energy_train, ref["energy_train"]), (rep.energy_holdout, ref["energy_holdout"])):
        scale = 2 * want[2] + want[3] + want[4]                          # (d2 is a difference: its error is relative to its parts)
        for g, w in zip(got[:2], want[:2]):
            assert abs(float(g) - w) <= 1e-12 * scale, (float(g), w)
        for g, w in zip(got[2:5], want[2:]):
            assert float(g) == pytest.approx(w, rel=1e-12), (float(g), w)
    plain = F.fidelity_report(tt, st)
    assert plain.energy_holdout is None and plain.aa_holdout is None and plain.privacy_loss is None and plain.closer_to_train is None
    assert plain.n_holdout is None and plain.aa == rep.aa and float(plain.energy_train.d2) == float(rep.energy_train.d2)
    ints = F.fidelity_report(tt.to(torch.int32), st.to(torch.int32), holdout=ht.to(torch.int32), probs=())
    assert ints.dcr_quantiles == () and ints.aa == rep.aa and ints.closer_to_train == rep.closer_to_train
    assert float(ints.energy_train.d2) == float(rep.energy_train.d2)


def test_example_flag_reports_the_synthetic_fidelity(gpu, capsys):
    spec = importlib.util.spec_from_file_location("ex_gmm_fidelity", os.path.join(ROOT, "examples", "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = argparse.Namespace(num_epochs=2, learning_rate=5e-2, batch_size=64, dimensions=2, num_samples=512, num_components=3, sigma=0.3,
                              synthetic_fidelity=True)
    mod.main(args)
    out = capsys.readouterr().out.splitlines()
    first = [ln for ln in out if ln.startswith("synthetic table")]
    second = [ln for ln in out if ln.startswith("distance to closest training record")]
    assert len(first) == 1 and len(second) == 1
    m = re.search(r"\((\d+) rows, d = 2\): energy distance to train ([0-9.eE+-]+) \((\d+) rows\), to test ([0-9.eE+-]+) \((\d+) rows\)", first[0])
    assert m and int(m.group(1)) == int(m.group(3)) == 512 and int(m.group(5)) == 512
    assert float(m.group(2)) >= 0 and float(m.group(4)) >= 0
    m = re.search(r"quantiles 5%/50%/95% ([0-9.]+)/([0-9.]+)/([0-9.]+), exact copies (\d+); adversarial accuracy train ([0-9.]+), held-out "
                  r"([0-9.]+), privacy loss (-?[0-9.]+)", second[0])
    assert m
    q5, q50, q95 = (float(m.group(i)) for i in (1, 2, 3))
    assert 0 <= q5 <= q50 <= q95 and int(m.group(4)) == 0
    aa, aah, loss = (float(m.group(i)) for i in (5, 6, 7))
    assert 0 <= aa <= 1 and 0 <= aah <= 1 and abs(loss - (aah - aa)) < 2e-4
    assert mod.parse_args(["--synthetic-fidelity"]).synthetic_fidelity is True and mod.parse_args([]).synthetic_fidelity is False
