"""Binned marginal counts and the marginal fidelity report on the GPU (d3p_marginals, d3p_amd.marginals) against tests/marginals_ref.py.
Everything the kernel produces is an integer: every count is compared BY VALUE with the numpy restatement, no tolerance and no case left
out.  Outputs and workspace are 0xFF-filled interiors between guards (tests/workspace_harness.py).  The shapes cross the strip of the
pair walk (S), the rows of a code workgroup (R), the pair tile (Pt) and the 64-column block of the code kernel; the lost-update cases put
every row of a strip on ONE cell.  The float64 summaries of the Python layer are held to 2 (K^2 + 4) 2^-53 of the restatement fed the
same counts."""
import argparse
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import marginals_ref as MR
from tests import workspace_harness as WH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 12345.0
ICANARY = 12345
PAD = 64


def np_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def LIB(gpu):
    import d3p_amd._lib as L
    return L.load()


@pytest.fixture(scope="module")
def SRP(LIB):
    """(S, R, Pt): the rows of a strip of the pair walk, the rows of a code workgroup, the pairs a workgroup holds at once."""
    return int(LIB.d3p_marginals_strip_rows()), int(LIB.d3p_marginals_code_rows()), int(LIB.d3p_marginals_pair_tile())


def entry(x, edges, nbins, B, pad=0, ws_fill="ones", ws_short=0, expect=0):
    """d3p_marginals on the numpy table x (n, d) with ld = d + pad (canaries in the padding), edges (d, >= B - 1) and nbins (d,) as the
    device will see them; outputs and workspace guarded and pre-filled: (one_way (d, K), two_way (P, K, K)) as int64 after the table,
    the guards and the paddings were checked -- or, with expect != 0, that return code with everything untouched."""
    import d3p_amd._lib as L
    lib = L.load()
    x = x[:, None] if x.ndim == 1 else x
    n, d = x.shape
    K, P = B + 1, d * (d - 1) // 2
    is_int = x.dtype == np.int32
    tdt, can = (torch.int32, ICANARY) if is_int else (torch.float32, CANARY)
    ld = d + pad
    xb = torch.full((n * ld + PAD,), can, dtype=tdt, device="cuda")
    xb.as_strided((n, d), (ld, 1)).copy_(torch.tensor(x))
    before = xb.clone()
    E = max(B - 1, 1)
    eb = torch.zeros((d, E), dtype=torch.float32)
    if B > 1:
        eb[:, :B - 1] = torch.tensor(np.asarray(edges, np.float32)[:, :B - 1])
    e_dev = eb.cuda()
    nb_dev = torch.tensor(np.asarray(nbins, np.int64).astype(np.uint32).view(np.int32)).cuda()                    # (uint32 words)
    meta = (e_dev.clone(), nb_dev.clone())
    one = WH.guarded(d * K * 4, "ones", "cuda")
    two = WH.guarded(max(P, 1) * K * K * 4, "ones", "cuda")
    need = int(lib.d3p_marginals_workspace(n, d, B))
    assert need == n * d
    ws = WH.guarded(need - ws_short, ws_fill, "cuda", seed=7)
    rc = lib.d3p_marginals(L.stream_ptr(), L.ptr(xb), int(is_int), ld, n, d, B, L.ptr(nb_dev), L.ptr(e_dev), L.ptr(one.interior),
                           L.ptr(two.interior) if P else None, L.ptr(ws.interior), need - ws_short)
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.d3p_last_error())
    assert torch.equal(xb.view(torch.int32), before.view(torch.int32)), "the table was written"
    assert torch.equal(e_dev.view(torch.int32), meta[0].view(torch.int32)) and torch.equal(nb_dev, meta[1]), "edges or nbins were written"
    for g, what in ((one, "one_way"), (two, "two_way"), (ws, "workspace")):
        g.check(what)
    if expect:
        assert bool((one.interior == 0xFF).all()) and bool((two.interior == 0xFF).all()), "a refused call wrote an output"
        assert torch.equal(ws.interior.cpu(), WH._fill_bytes(ws.nbytes, ws_fill, seed=7)), "a refused call wrote the workspace"
        return None
    o = np_(one.interior.view(torch.int32)).astype(np.int64).reshape(d, K) & 0xFFFFFFFF
    if not P:
        assert bool((two.interior == 0xFF).all()), "d = 1 has no pairs: two_way is not touched"
        return o, np.zeros((0, K, K), np.int64)
    return o, np_(two.interior.view(torch.int32)).astype(np.int64).reshape(P, K, K) & 0xFFFFFFFF


def consistent(one, two, n, d):
    """The properties that hold by value whatever the data: every table sums to n, and a pair's table has the one-way counts of its
    columns as its row and column sums."""
    assert (one.sum(axis=1) == n).all() and (two.sum(axis=(1, 2)) == n).all()
    pr = MR.pairs(d)
    assert np.array_equal(two.sum(axis=2), one[pr[:, 0]]) and np.array_equal(two.sum(axis=1), one[pr[:, 1]])


def table(seed, n, d, is_int):
    """A table with values ON edges (the edges below are values of the table), NaN and +-inf sprinkled in."""
    rng = np.random.default_rng(seed)
    if is_int:
        return rng.integers(-6, 7, (n, d)).astype(np.int32)
    x = np.round(rng.normal(size=(n, d)) * 4).astype(np.float32) / np.float32(4)       # a grid: ties with the edges are frequent
    x[rng.random((n, d)) < 0.02] = np.nan
    x[rng.random((n, d)) < 0.01] = np.inf
    x[rng.random((n, d)) < 0.01] = -np.inf
    x[rng.random((n, d)) < 0.02] = -0.0
    return x


def cuts(seed, x, B):
    """Per-column bin counts in [1, B] -- the first column B, the last 1 -- and sorted edges drawn from the column's own finite values
    (so values lie exactly on edges) with duplicates (so bins are empty)."""
    rng = np.random.default_rng(seed)
    n, d = x.shape
    nb = rng.integers(1, B + 1, d)
    nb[0], nb[-1] = B, 1 if d > 1 else B
    e = np.zeros((d, max(B - 1, 1)), np.float32)
    for c in range(d):
        col = x[:, c].astype(np.float32)
        fin = col[np.isfinite(col)]
        pool = fin if len(fin) else np.zeros(1, np.float32)
        e[c, :B - 1] = np.sort(rng.choice(pool, B - 1)) if B > 1 else 0
        e[c, nb[c] - 1:] = 777.0                     # beyond nb_c - 1: never looked at
    return e, nb


def by_value(x, e, nb, B, pad=0, **kw):
    one, two = entry(x, e, nb, B, pad, **kw)
    want = MR.counts_product(x, e, nb, B)
    assert np.array_equal(one, want[0]), "one_way"
    assert np.array_equal(two, want[1]), "two_way"
    consistent(one, two, x.shape[0], x.shape[1])
    return one, two


# ------------------------------------------------------------------------------------------------ the shapes, crossed sparsely
def _sweep(S, R, Pt):
    ns = (1, 2, 63, 64, 65, R - 1, R, R + 1, S - 1, S, S + 1, 2 * S + 1)
    want_pairs = (0, 1, Pt - 1, Pt, Pt + 1, 2 * Pt + 1)
    ds = sorted({min(range(1, 4 * Pt + 4), key=lambda d: (abs(d * (d - 1) // 2 - p), d)) for p in want_pairs} | {1, 2, 3})
    Bs = (1, 2, 3, 31, 32)
    cases = [(n, ds[i % len(ds)], Bs[i % 5]) for i, n in enumerate(ns)]
    cases += [(n, ds[(i + 2) % len(ds)], Bs[(i + 3) % 5]) for i, n in enumerate(ns)]
    cases += [(n, ds[-1], 32) for n in (S + 1, 65)] + [(65, d, B) for d in ds for B in Bs]
    cases += [(65, 63, 3), (66, 64, 2), (130, 65, 31), (67, 129, 1), (R + 1, 65, 2), (3, 33, 32), (5, 17, 16), (9, 9, 16)]   # the 64-column block
    return list(dict.fromkeys(cases))


def test_sweep_by_value(SRP):
    S, R, Pt = SRP
    cases = _sweep(S, R, Pt)
    assert {d * (d - 1) // 2 for _, d, _ in cases} >= {0, 1, 3, 6, 10}
    for i, (n, d, B) in enumerate(cases):
        x = table(100 + i, n, d, i % 2 == 1)
        e, nb = cuts(500 + i, x, B)
        by_value(x, e, nb, B, pad=(0, 1, 7, 0, 3)[i % 5])


def test_the_vae_width(SRP):
    """784 binary columns at B = 2, 65 rows: 306 936 pair tables."""
    rng = np.random.default_rng(7)
    x = (rng.random((65, 784)) < 0.3).astype(np.int32)
    x[:, 5] = 0                                         # a dead pixel
    e = np.zeros((784, 1), np.float32)
    nb = np.full(784, 2)
    nb[9] = 1
    one, two = by_value(x, e, nb, 2, pad=16)
    assert one[5].tolist() == [65, 0, 0] and one[9].tolist() == [65, 0, 0] and two.shape == (784 * 783 // 2, 3, 3)


# ------------------------------------------------------------------------------------------------ lost updates
def test_every_row_on_one_cell(SRP):
    """n = 70 000 equal rows: every lane of every wavefront adds to the SAME cell of its pair, and that cell must hold exactly n (above
    2^16, across three strips)."""
    S, R, Pt = SRP
    n, d = 70000, 5
    assert n > 2 * S and n > 2 ** 16
    for B, row in ((16, [0.5, -3.0, np.nan, 1e30, 0.0]), (2, [1.0, 1.0, 0.0, np.nan, -np.inf]), (32, [3.0, 3.0, 3.0, 3.0, 3.0])):
        x = np.tile(np.array(row, np.float32), (n, 1))
        e = np.tile(np.linspace(-4, 4, max(B - 1, 1), dtype=np.float32), (d, 1))
        nb = np.full(d, B)
        one, two = by_value(x, e, nb, B)
        assert (one.max(axis=1) == n).all() and (two.max(axis=(1, 2)) == n).all() and (np.count_nonzero(two, axis=(1, 2)) == 1).all()
        assert one[2, B] == (n if np.isnan(row[2]) else 0)


def test_two_alternating_rows_and_a_missing_column(SRP):
    S, R, Pt = SRP
    n, d, B = 2 * S + 3, 4, 3
    x = np.zeros((n, d), np.float32)
    x[0::2] = (-1.0, 0.0, 5.0, np.nan)
    x[1::2] = (2.0, 0.0, -5.0, np.nan)                  # column 1 constant, column 3 all NaN
    e = np.tile(np.array([[-0.5, 0.5]], np.float32), (d, 1))
    one, two = by_value(x, e, np.full(d, B), B, pad=2)
    half = (n + 1) // 2
    assert one[0].tolist() == [half, 0, n - half, 0] and one[1].tolist() == [0, n, 0, 0] and one[3].tolist() == [0, 0, 0, n]
    p = MR.pair_index(0, 2, d)
    assert two[p, 0, 2] == half and two[p, 2, 0] == n - half and two[p].sum() == n
    assert two[MR.pair_index(2, 3, d), :, B].tolist() == [n - half, 0, half, 0]


# ------------------------------------------------------------------------------------------------ independence, by equality
def test_counts_depend_on_the_arguments_alone(SRP):
    S, R, Pt = SRP
    n, d, B = S + 77, 5, 16
    x = table(20, n, d, False)
    e, nb = cuts(21, x, B)
    base = by_value(x, e, nb, B)
    for other in (entry(x, e, nb, B),                                       # a repeat
                  entry(x, e, nb, B, pad=5),                                # another row stride
                  entry(x, e, nb, B, ws_fill="zero"), entry(x, e, nb, B, ws_fill="bits"), entry(x, e, nb, B, ws_fill="big"),   # what the workspace held
                  entry(x[np.random.default_rng(22).permutation(n)], e, nb, B)):                                             # the order of the rows
        assert np.array_equal(other[0], base[0]) and np.array_equal(other[1], base[1])
    xi = table(23, 2 * R + 1, 3, True)
    ei, nbi = cuts(24, xi, 31)
    a, b = by_value(xi, ei, nbi, 31), entry(xi.astype(np.float32), ei, nbi, 31, pad=1)                                       # int32 converts exactly
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ hostile device metadata
def test_hostile_nbins_and_unsorted_edges_stay_in_range(SRP):
    """nbins of 0 and 2^32 - 1 and edges in no order: the kernel clamps and bounds its search, so the call returns, every row lands in
    one of the K cells of its table (the tables still sum to n, with the one-way counts as their margins) and no guard is touched."""
    S, R, Pt = SRP
    n, d = R + 9, 6
    x = table(30, n, d, False)
    rng = np.random.default_rng(31)
    for B in (1, 2, 32):
        e = rng.normal(size=(d, max(B - 1, 1))).astype(np.float32)           # unsorted
        e[1, :] = np.nan
        e[2, 0] = np.inf
        nb = np.array([0, 2 ** 32 - 1, 0, 2 ** 31, B, 1], np.int64)
        one, two = entry(x, e, nb, B, pad=1)
        consistent(one, two, n, d)
        assert one.shape == (d, B + 1) and (one >= 0).all() and (two >= 0).all()
        nan_rows = np.isnan(x).sum(axis=0)
        assert np.array_equal(one[:, B], nan_rows)                           # the missing cell does not depend on the edges
        assert one[0, 0] == n - nan_rows[0] and one[2, 0] == n - nan_rows[2] and one[5, 0] == n - nan_rows[5]     # 0 clamps to one bin
    e, nb = cuts(32, x, 8)
    e = e[:, ::-1].copy()                                                    # decreasing edges under valid nbins
    one, two = entry(x, e, nb, 8)
    consistent(one, two, n, d)


# ------------------------------------------------------------------------------------------------ the workspace
def test_a_short_workspace_is_refused_with_everything_untouched(SRP):
    x = table(40, 100, 3, False)
    e, nb = cuts(41, x, 4)
    for fill in ("ones", "bits"):
        assert entry(x, e, nb, 4, ws_fill=fill, ws_short=1, expect=-4) is None


@pytest.mark.parametrize("fill", ["zero", "ones", "bits"])
def test_the_python_layer_on_guarded_memory(LIB, SRP, monkeypatch, fill):
    import d3p_amd._lib as L
    from d3p_amd import marginals as M
    S, R, Pt = SRP
    x = table(50, R + 5, 4, False)
    e, nb = cuts(51, x, 8)
    be = M.BinEdges(torch.tensor(e), torch.tensor(nb, dtype=torch.int64), 8)
    xt = torch.tensor(x).cuda()
    want = MR.counts(x, e, nb, 8)
    rec = WH.Recorder(fill, 0, None)
    WH.guarded_empty(monkeypatch, M, rec, "marginals")
    got = M.marginal_counts(xt, be)
    torch.cuda.synchronize()
    rec.check_all("marginal_counts")
    assert [g.nbytes for g in rec.workspaces] == [(R + 5) * 4] and len(rec.buffers) == 3
    assert got.one_way.dtype == got.two_way.dtype == got.pairs.dtype == torch.int64 and got.n == R + 5
    assert np.array_equal(np_(got.one_way), want[0]) and np.array_equal(np_(got.two_way), want[1]) and np.array_equal(np_(got.pairs), MR.pairs(4))
    short = WH.Recorder(fill, 1, None)
    WH.guarded_empty(monkeypatch, M, short, "marginals")
    with pytest.raises(L.D3PError, match="workspace too small"):
        M.marginal_counts(xt, be)
    torch.cuda.synchronize()
    short.check_all("short")
    for g in short.buffers:                                                  # outputs and workspace as they were handed out
        assert torch.equal(g.interior.cpu(), WH._fill_bytes(g.nbytes, g.fill, seed=g.seed)), g.tag


# ------------------------------------------------------------------------------------------------ the Python layer
def test_python_layer_on_the_device(gpu, SRP):
    from d3p_amd import marginals as M
    x = table(60, 300, 3, True)
    xt = torch.tensor(x).cuda()
    wide = torch.zeros((300, 7), dtype=torch.int32, device="cuda")
    wide[:, :3] = xt
    be = M.bin_edges(xt, bins=13, kind="integer")
    assert be.max_bins == 13 and be.nbins.tolist() == [13, 13, 13] and be.edges[0].tolist() == [float(v) for v in range(-6, 6)]
    got = M.marginal_counts(wide[:, :3], be)                                 # a strided view
    want = MR.counts(x, np_(be.edges), be.nbins.tolist(), 13)
    assert np.array_equal(np_(got.one_way), want[0]) and np.array_equal(np_(got.two_way), want[1])
    assert np.array_equal(np_(got.one_way)[0, :13], np.bincount(x[:, 0] + 6, minlength=13))     # one bin per integer
    with pytest.raises(ValueError, match="need 13 bins, above bins = 12"):
        M.bin_edges(xt, bins=12, kind="integer")
    with pytest.raises(ValueError, match="integral-valued"):
        M.bin_edges(xt.float() + 0.5, kind="integer")
    one_d = M.marginal_counts(xt[:, 0], M.bin_edges(xt[:, 0], bins=13, kind="integer"))       # the 1-D form: d = 1, no pairs
    assert one_d.two_way.shape == (0, 14, 14) and one_d.pairs.shape == (0, 2) and np.array_equal(np_(one_d.one_way)[0], want[0][0])
    for v in (2 ** 24 + 1, -2 ** 24 - 1):
        big = xt.clone()
        big[2, 1] = v
        with pytest.raises(ValueError, match="beyond 2\\^24"):
            M.marginal_counts(big, be)
        with pytest.raises(ValueError, match="beyond 2\\^24"):
            M.bin_edges(big)
    # the quantile and the uniform rule against the restatement
    f = table(61, 1001, 4, False)
    f[:, 2] = np.where(np.arange(1001) % 3 == 0, 1.0, 0.0)                     # two distinct values: two bins
    f[:, 3] = np.nan                                                          # nothing finite: one bin
    ft = torch.tensor(f).cuda()
    for bins in (1, 2, 16, 32):
        q = M.bin_edges(ft, bins=bins)
        assert q.max_bins == bins and q.edges.shape == (4, max(bins - 1, 1)) and not q.edges.is_cuda
        for c in range(4):
            ref = MR.quantile_edges(f[:, c], bins)
            assert q.nbins[c] == len(ref) + 1 and q.edges[c, :len(ref)].tolist() == ref and not q.edges[c, len(ref):].any(), (bins, c)
        assert q.nbins[3] == 1 and q.nbins[2] == (2 if bins > 1 else 1)
    u = M.bin_edges(ft, bins=8, kind="uniform")
    fin = f[:, 0][np.isfinite(f[:, 0])].astype(np.float64)
    assert u.nbins.tolist() == [8, 8, 8, 1]
    assert u.edges[0].tolist() == [float(np.float32(fin.min() + (fin.max() - fin.min()) * k / 8)) for k in range(1, 8)]


def test_marginal_fidelity_against_the_restatement(gpu, SRP):
    from d3p_amd import marginals as M
    rng = np.random.default_rng(70)
    real = rng.normal(size=(1500, 4)).astype(np.float32)
    real[:, 1] = real[:, 0] + np.float32(0.5) * real[:, 1]                     # an association the synthetic table lacks
    synth = rng.normal(size=(1100, 4)).astype(np.float32)
    synth[::50, 2] = np.nan
    hold = rng.normal(size=(700, 4)).astype(np.float32)
    hold[:, 1] = hold[:, 0] + np.float32(0.5) * hold[:, 1]
    rt, st, ht = (torch.tensor(v).cuda() for v in (real, synth, hold))
    for bins in (3, 16):
        K = bins + 1
        bound = 2 * (K * K + 4) * 2.0 ** -53
        rep = M.marginal_fidelity(rt, st, bins=bins, holdout=ht, top=3)
        be = rep.edges
        e, nb = np_(be.edges), be.nbins.tolist()
        for c in range(4):
            assert be.edges[c, :nb[c] - 1].tolist() == MR.quantile_edges(real[:, c], bins)
        cr, cs, ch = (MR.counts_product(v, e, nb, bins) for v in (real, synth, hold))
        for t, c in ((rt, cr), (st, cs), (ht, ch)):                           # the counts, by value
            got = M.marginal_counts(t, be)
            assert np.array_equal(np_(got.one_way), c[0]) and np.array_equal(np_(got.two_way), c[1])
        for r, other, n_other in ((rep, cs, 1100), (rep.floor, ch, 700)):
            ref = MR.summaries(cr[0], cr[1], 1500, other[0], other[1], n_other)
            for k in ("tvd_one_way", "tvd_two_way"):
                err = np.abs(np_(getattr(r, k)) - ref[k]).max()
                print(f"bins {bins}: {k} largest difference {err:.3e} (bound {bound:.3e})")
                assert err <= bound, (k, err, bound)
            assert r.tvd_one_way_mean == pytest.approx(ref["tvd_one_way_mean"], rel=1e-13) and r.tvd_two_way_mean == pytest.approx(ref["tvd_two_way_mean"], rel=1e-13)
            assert np.allclose(np_(r.cramers_v_real), ref["cramers_v_a"], rtol=1e-12, atol=1e-15)
            assert np.allclose(np_(r.cramers_v_synthetic), ref["cramers_v_b"], rtol=1e-12, atol=1e-15)
            assert r.assoc_diff_mean == pytest.approx(ref["assoc_diff_mean"], rel=1e-11) and r.assoc_diff_max == pytest.approx(ref["assoc_diff_max"], rel=1e-11)
            assert np.array_equal(np_(r.missing_real), ref["missing_a"]) and np.array_equal(np_(r.missing_synthetic), ref["missing_b"])
            assert (r.n_real, r.n_synthetic) == (1500, n_other) and r.columns == (0, 1, 2, 3) and len(r.worst_columns) == 3 and len(r.worst_pairs) == 3
            assert r.worst_pairs[0][1] == float(np_(r.tvd_two_way).max()) and r.worst_columns[0][1] == float(np_(r.tvd_one_way).max())
        assert rep.floor.floor is None and rep.worst_pairs[0][0] == (0, 1)    # the pair whose association is missing
        assert rep.tvd_two_way_mean > rep.floor.tvd_two_way_mean and rep.assoc_diff_max > rep.floor.assoc_diff_max
        assert float(rep.missing_synthetic[2]) == 22 / 1100
    same = M.marginal_fidelity(rt, rt.clone(), bins=16)
    assert same.floor is None and bool((same.tvd_one_way == 0).all()) and bool((same.tvd_two_way == 0).all())
    assert same.tvd_one_way_mean == 0.0 and same.tvd_two_way_mean == 0.0 and same.assoc_diff_max == 0.0
    sub = M.marginal_fidelity(rt, st, bins=16, columns=[3, 0], top=0)         # a subset, in the caller's order and by the caller's ids
    full = M.marginal_fidelity(rt, st, bins=16)
    assert sub.columns == (3, 0) and sub.worst_columns == () and sub.worst_pairs == () and sub.tvd_two_way.shape == (1,)
    assert float(sub.tvd_one_way[0]) == pytest.approx(float(full.tvd_one_way[3]), rel=1e-13)
    assert float(sub.tvd_one_way[1]) == pytest.approx(float(full.tvd_one_way[0]), rel=1e-13)
    assert float(sub.tvd_two_way[0]) == pytest.approx(float(full.tvd_two_way[MR.pair_index(0, 3, 4)]), rel=1e-13)   # the transposed table
    one = M.marginal_fidelity(rt[:, 0], st[:, 0], bins=4)                     # d = 1: no pairs
    assert one.tvd_two_way.shape == (0,) and np.isnan(one.tvd_two_way_mean) and np.isnan(one.assoc_diff_mean) and one.worst_pairs == ()
    given = M.marginal_fidelity(rt, st, bins=[[0.0], [-1.0, 1.0], [], [0.0, 0.0]])
    assert given.edges.max_bins == 3 and given.edges.nbins.tolist() == [2, 3, 1, 3] and float(given.tvd_one_way[2]) == pytest.approx(22 / 1100, rel=1e-13)


def test_example_flag_reports_the_marginal_fidelity(gpu, capsys):
    spec = importlib.util.spec_from_file_location("ex_gmm_marginals", os.path.join(ROOT, "examples", "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = argparse.Namespace(num_epochs=2, learning_rate=5e-2, batch_size=64, dimensions=2, num_samples=512, num_components=3, sigma=0.3,
                              synthetic_fidelity=True, marginal_fidelity=8)
    mod.main(args)
    out = capsys.readouterr().out.splitlines()
    first = [ln for ln in out if ln.startswith("binned marginals")]
    second = [ln for ln in out if ln.startswith("association (Cramer's V)")]
    assert len(first) == 1 and len(second) == 1
    num = r"([0-9.]+)"
    m = re.search(r"\(8 bins, 2 columns, 512 synthetic rows\): 1-way TVD mean " + num + r", worst column ([01]) \(" + num + r"\); 2-way TVD mean " + num +
                  r", worst columns 0 and 1 \(" + num + r"\)", first[0])
    assert m
    t1, w1, t2, w2 = float(m.group(1)), float(m.group(3)), float(m.group(4)), float(m.group(5))
    assert 0 <= t1 <= w1 <= 1 and 0 <= t2 <= 1 and abs(t2 - w2) < 1e-4       # one pair: its TVD is the mean
    m = re.search(r"difference mean " + num + ", max " + num + r"; held-out floor \(512 rows\): 1-way TVD mean " + num + ", 2-way TVD mean " + num +
                  ", association difference mean " + num, second[0])
    assert m and all(0 <= float(g) <= 1 for g in m.groups()) and abs(float(m.group(1)) - float(m.group(2))) < 1e-4
    # the two lines of --synthetic-fidelity are as they were
    old = [ln for ln in out if ln.startswith("synthetic table") or ln.startswith("distance to closest training record")]
    assert len(old) == 2
    assert re.search(r"\(512 rows, d = 2\): energy distance to train [0-9.eE+-]+ \(512 rows\), to test [0-9.eE+-]+ \(512 rows\)$", old[0])
    assert re.search(r"quantiles 5%/50%/95% [0-9.]+/[0-9.]+/[0-9.]+, exact copies \d+; adversarial accuracy train [0-9.]+, held-out [0-9.]+, "
                     r"privacy loss -?[0-9.]+$", old[1])
    assert mod.parse_args(["--marginal-fidelity"]).marginal_fidelity == 16 and mod.parse_args(["--marginal-fidelity", "4"]).marginal_fidelity == 4
    assert mod.parse_args([]).marginal_fidelity is None and mod.parse_args(["--synthetic-fidelity"]).marginal_fidelity is None
