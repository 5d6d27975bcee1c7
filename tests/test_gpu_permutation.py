"""The label sums and the energy distance's permutation test on the GPU (d3p_pair_label_sums, d3p_amd.permutation) against
tests/permutation_ref.py.  The restatement adds in the kernel's stated order, so s11, s1t and n1 are compared BY VALUE: on tables whose
float32 chain the numpy emulation reproduces exactly (integers, and floats on a grid of 2^-8, where every t^2 + q fits a float64 and the
emulated fmaf rounds once), and within the DERIVED bound of the exact comparator on the hostile tables.  Everything the contract calls
independent -- R, the labelling's column and neighbours, ld, what the workspace held, a repeat, the bits of rows beyond m -- is compared
bit for bit.  The table, the labels and the row sums carry canaries and are checked unchanged; outputs and workspace lie between guards
(tests/workspace_harness.py) and are filled with 0xFF bytes before every call.  There is one form."""
import argparse
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import fidelity_ref as FR
from tests import permutation_ref as PR
from tests import workspace_harness as WH
from tests.test_permutation_host import _cases, _fixed, _labels, words

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 12345.0
ICANARY = 12345
PAD = 64
T, S = PR.T, PR.S
_REF = {}      # case name -> the restatement / the exact comparator: computed once, shared, never changed


def np_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def LIB(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    assert lib.d3p_pair_label_sums_tile_rows() == T
    return lib


def u32(a):
    """A numpy uint32 array as a CUDA uint32 tensor."""
    return torch.tensor(np.ascontiguousarray(a).view(np.int32)).cuda().view(torch.uint32)


def entry(z, labels, row_sum, pad=0, fill="ones", short_by=0, expect=0):
    """d3p_pair_label_sums on the numpy table z (m, d) with ld = d + pad, canaries in the padding; the outputs and the workspace between
    guards, pre-filled: {"s11", "s1t", "n1"} after the inputs and the guards were checked.  With short_by the workspace is that many
    bytes short: the return code is `expect` and everything must be as it was handed out."""
    import d3p_amd._lib as L
    lib = L.load()
    z = z[:, None] if z.ndim == 1 else z
    m, d = z.shape
    R = labels.shape[1]
    assert labels.shape[0] == -(-m // T) and labels.dtype == np.uint32 and row_sum.shape == (m,)
    is_int = z.dtype == np.int32
    tdt, can = (torch.int32, ICANARY) if is_int else (torch.float32, CANARY)
    ld = d + pad
    zb = torch.full((m * ld + PAD,), can, dtype=tdt, device="cuda")
    zb.as_strided((m, d), (ld, 1)).copy_(torch.tensor(z))
    lb, rb = u32(labels), torch.tensor(row_sum, dtype=torch.float64).cuda()
    before = (zb.clone(), lb.view(torch.int32).clone(), rb.clone())
    rec = WH.Recorder(fill, short_by, None)
    outs = [rec.take(R * w, "cuda", f"out{i}", output=True) for i, w in enumerate((8, 8, 4))]
    need = int(lib.d3p_pair_label_sums_workspace(m, d, R))
    assert need == 8 * R * -(-m // T)
    ws = rec.take(need, "cuda", "ws")
    rc = lib.d3p_pair_label_sums(L.stream_ptr(), L.ptr(zb), int(is_int), ld, m, d, R, L.ptr(lb), L.ptr(rb), L.ptr(outs[0].interior),
                                 L.ptr(outs[1].interior), L.ptr(outs[2].interior), L.ptr(ws.interior), ws.nbytes)
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.d3p_last_error())
    rec.check_all("d3p_pair_label_sums")
    assert torch.equal(zb.view(torch.int32), before[0].view(torch.int32)) and torch.equal(lb.view(torch.int32), before[1]) and \
        torch.equal(WH.raw_bytes(rb), WH.raw_bytes(before[2])), "an input was written"
    if expect != 0:
        for g in rec.buffers:
            assert torch.equal(g.interior.cpu(), WH._fill_bytes(g.nbytes, g.fill, seed=g.seed)), g.tag
        return None
    return {"s11": np_(outs[0].interior.view(torch.float64)).copy(), "s1t": np_(outs[1].interior.view(torch.float64)).copy(),
            "n1": np_(outs[2].interior.view(torch.int32)).astype(np.int64) & 0xFFFFFFFF}


def same_bits(a, b):
    return a.tobytes() == b.tobytes()


def grid_table(seed, m, d, is_int):
    """A table whose float32 chain the numpy emulation reproduces exactly: integers, or normals on a grid of 2^-8."""
    rng = np.random.default_rng(seed)
    if is_int:
        return rng.integers(-50, 51, (m, d)).astype(np.int32)
    return (np.round(rng.normal(size=(m, d)) * 256.0) / 256.0).astype(np.float32)


def row_sums_like(seed, m):
    """Some caller's row sums: s1t is defined on whatever they hold."""
    return np.abs(np.random.default_rng(seed).normal(size=m)) * 100.0


# ------------------------------------------------------------------------------------------------ by value against the restatement
def _sweep():
    ms = (2, T - 1, T, T + 1, 2 * T + 1, S - 1, S, S + 1, 2 * S + 1)
    Rs = (1, 2, 63, 64, 65, 129)
    ds = (1, 2, 3, 31, 32, 33, 65)
    cases = [(m, Rs[i % len(Rs)], ds[i % len(ds)]) for i, m in enumerate(ms)]
    cases += [(T + 1, R, ds[(i + 3) % len(ds)]) for i, R in enumerate(Rs)]
    cases += [(2 * T + 1, Rs[(i + 2) % len(Rs)], d) for i, d in enumerate(ds)]
    cases += [(2 * S + 1, 129, 33), (S + 1, 65, 2), (2 * T + 1, 65, 784)]
    return list(dict.fromkeys(cases))


def test_sweep_by_value_against_the_restatement(LIB):
    rng = np.random.default_rng(40)
    for i, (m, R, d) in enumerate(_sweep()):
        is_int = i % 2 == 1
        z = grid_table(100 + i, m, d, is_int)
        lab = PR.pack(_labels(rng, m, R))
        t = row_sums_like(200 + i, m)
        if i not in _REF:
            _REF[i] = PR.restate(z, lab, t)
        want = _REF[i]
        got = entry(z, lab, t, pad=(0, 1, 7, 4)[i % 4])
        for k in ("n1", "s1t", "s11"):
            assert np.array_equal(got[k], want[k]), (m, R, d, is_int, k, got[k], want[k])


def test_exact_cases_by_value_against_python_integers(LIB):
    rng = np.random.default_rng(41)
    m = 2 * S + 5
    bits = _labels(rng, m, 70)
    bits[0] = False                      # no row: s11 = 0, n1 = 0
    bits[1] = False
    bits[1, S + 1] = True                # one row: the diagonal is +0.0
    lab = PR.pack(bits)
    t = row_sums_like(3, m)
    # d = 1, integer coordinates (both dtypes): every distance an integer, every float64 sum exact in any order
    k = rng.integers(-400, 401, m)       # (|k_i - k_j| <= 800: 25 x 800^2 < 2^24, so the lattice's q is exact in float32 too)
    want = [int(np.abs(k[g][:, None] - k[g][None, :]).sum()) for g in bits]                  # Python integers
    assert want[0] == 0 and want[1] == 0 and max(want) > 10 ** 6
    for z in (k.astype(np.int32), k.astype(np.float32)):
        got = entry(z, lab, t, pad=3)
        assert got["s11"].tolist() == [float(w) for w in want] and got["n1"].tolist() == bits.sum(axis=1).tolist()
        assert got["s11"][0] == 0.0 and got["n1"][0] == 0 and got["s11"][1] == 0.0 and got["n1"][1] == 1
        assert not np.signbit(got["s11"][:2]).any()
    # d = 2 on a 3-4-5 lattice: row i is k_i (3, 4), every distance 5 |k_i - k_j|
    z = (k[:, None] * np.array([3, 4])).astype(np.float32)
    got = entry(z, lab, t)
    assert got["s11"].tolist() == [float(5 * w) for w in want]


def test_all_ones_labels_agree_with_the_sum_of_the_row_sums(LIB):
    from d3p_amd import fidelity as F
    for m, d in ((S + 3, 5), (2 * T + 1, 33)):
        z = np.random.default_rng(m).normal(size=(m, d)).astype(np.float32)
        t = np_(F.pair_stats(torch.tensor(z).cuda(), torch.tensor(z).cuda(), True)["sum"])
        got = entry(z, PR.pack(np.ones((3, m), bool)), t)
        total = FR._fsum(t)
        assert (np.abs(got["s11"] - total) <= (m + PR.chain(m) + 4) * 2.0 ** -53 * total).all(), (got["s11"], total)
        assert (np.abs(got["s1t"] - total) <= (m + 2) * 2.0 ** -53 * total).all() and got["n1"].tolist() == [m] * 3


# ------------------------------------------------------------------------------------------------ independence, bit for bit
def test_a_labellings_bits_depend_on_that_labelling_alone(LIB):
    rng = np.random.default_rng(42)
    m, d = 2 * S + 7, 5
    z = rng.normal(size=(m, d)).astype(np.float32)
    t = row_sums_like(4, m)
    R = 200
    bits = _labels(rng, m, R)
    bits[0] = bits[64] = np.arange(m) >= m // 3           # the identity labelling at r = 0 and at r = 64
    lab = PR.pack(bits)
    base = entry(z, lab, t)
    for k in ("s11", "s1t", "n1"):
        assert base[k][0] == base[k][64], k
    assert same_bits(base["s11"][:1], base["s11"][64:65])
    # a repeat; another ld; other workspace fills
    for pad, fill in ((0, "ones"), (3, "zero"), (0, "big"), (9, "bits")):
        again = entry(z, lab, t, pad=pad, fill=fill)
        assert all(same_bits(again[k], base[k]) for k in ("s11", "s1t", "n1")), (pad, fill)
    # other columns, other neighbours, another R: labelling r of the base run at column c of the new one
    for R2, moves in ((1, {0: 77}), (65, {3: 0, 64: 130, 0: 131, 17: 199}), (513, {512: 5, 100: 64, 511: 199})):
        other = _labels(np.random.default_rng(R2), m, R2)
        for c, r in moves.items():
            other[c] = bits[r]
        got = entry(z, PR.pack(other), t, pad=1)
        for c, r in moves.items():
            assert all(same_bits(got[k][c:c + 1], base[k][r:r + 1]) for k in ("s11", "s1t", "n1")), (R2, c, r)
    # every bit of a row beyond m set: nothing changes
    hostile = lab.copy()
    hostile[-1] |= np.uint32((0xFFFFFFFF << (m % T)) & 0xFFFFFFFF)
    assert not np.array_equal(hostile, lab)
    got = entry(z, hostile, t)
    assert all(same_bits(got[k], base[k]) for k in ("s11", "s1t", "n1"))


# ------------------------------------------------------------------------------------------------ special values, the workspace
def test_non_finite_input_makes_every_s11_nan(LIB):
    rng = np.random.default_rng(43)
    m, d = S + 9, 35
    z = rng.normal(size=(m, d)).astype(np.float32)
    bits = _labels(rng, m, 66)
    lab = PR.pack(bits)
    t = row_sums_like(5, m)
    clean = entry(z, lab, t)
    assert np.isfinite(clean["s11"]).all()
    for i, c, v in ((0, 0, np.nan), (m - 1, d - 1, np.inf), (T + 2, 33, -np.inf)):
        zz = z.copy()
        zz[i, c] = v
        if np.isnan(v):
            zz[i, :] = v                                   # a whole NaN row
        got = entry(zz, lab, t, pad=2)                     # (returns: the call came back and no guard was touched)
        assert np.isnan(got["s11"]).all(), (i, c, v)
        assert np.array_equal(got["n1"], bits.sum(axis=1)) and same_bits(got["s1t"], clean["s1t"])
    zz = z.copy()
    zz[7, 1] = 3e38                                        # finite; q overflows: IEEE
    got = entry(zz, lab, t)
    sel = bits[:, 7] & (bits.sum(axis=1) > 1)
    assert np.isinf(got["s11"][sel]).all() and same_bits(got["s11"][~sel], clean["s11"][~sel]) and sel.any() and (~sel).any()
    tt = t.copy()
    tt[3] = np.nan                                         # s1t propagates what the selected rows hold
    got = entry(z, lab, tt)
    assert np.array_equal(np.isnan(got["s1t"]), bits[:, 3]) and same_bits(got["s11"], clean["s11"])


def test_a_short_workspace_is_refused_with_everything_untouched(LIB):
    z = grid_table(9, 2 * T + 1, 3, False)
    lab = PR.pack(_labels(np.random.default_rng(44), 2 * T + 1, 65))
    for fill in ("ones", "bits"):
        assert entry(z, lab, row_sums_like(6, 2 * T + 1), fill=fill, short_by=1, expect=-4) is None
        assert b"workspace too small" in LIB.d3p_last_error()


@pytest.mark.parametrize("fill", ["zero", "ones", "bits"])
def test_workspace_contents_and_extent_through_the_python_layer(LIB, monkeypatch, fill):
    import d3p_amd._lib as L
    from d3p_amd import permutation as P
    m, d, R = S + 3, 5, 70
    z = torch.tensor(grid_table(10, m, d, False)).cuda()
    lab = u32(PR.pack(_labels(np.random.default_rng(45), m, R)))
    t = torch.tensor(row_sums_like(7, m)).cuda()
    want = P.label_sums(z, lab, t)
    rec = WH.Recorder(fill, 0, None)
    WH.guarded_empty(monkeypatch, P, rec, "label_sums")
    got = P.label_sums(z, lab, t)
    torch.cuda.synchronize()
    rec.check_all("label_sums")
    assert [g.nbytes for g in rec.workspaces] == [8 * R * -(-m // T)] and len(rec.buffers) == 4
    for k in ("s11", "s1t", "n1"):
        assert torch.equal(WH.raw_bytes(getattr(got, k)), WH.raw_bytes(getattr(want, k))), (fill, k)
    short = WH.Recorder(fill, 1, None)
    WH.guarded_empty(monkeypatch, P, short, "label_sums")
    with pytest.raises(L.D3PError, match="workspace too small"):
        P.label_sums(z, lab, t)
    torch.cuda.synchronize()
    short.check_all("short")
    for g in short.buffers:                                # outputs and workspace as they were handed out
        assert torch.equal(g.interior.cpu(), WH._fill_bytes(g.nbytes, g.fill, seed=g.seed)), g.tag


# ------------------------------------------------------------------------------------------------ within the bound
@pytest.mark.parametrize("name,z", list(_cases()), ids=[c[0] for c in _cases()])
def test_hostile_tables_within_the_bound_of_the_exact_comparator(LIB, name, z):
    m = z.shape[0]
    d = z.shape[1] if z.ndim == 2 else 1
    bits = _labels(np.random.default_rng(5), m, 13)
    lab = PR.pack(bits)
    if name not in _REF:
        _REF[name] = PR.exact(z, lab)
    ex = _REF[name]
    tol = PR.bound(ex, m, d)
    got = entry(z, lab, row_sums_like(8, m), pad=1)
    err = np.abs(got["s11"] - ex)
    assert (err <= tol).all(), (name, float((err[tol > 0] / tol[tol > 0]).max()))
    assert (got["s11"][tol == 0] == 0.0).all()
    print(f"{name}: largest error / bound {float((err[tol > 0] / tol[tol > 0]).max()):.4f}")


# ------------------------------------------------------------------------------------------------ the Python layer, the test
def test_python_layer_on_the_device(LIB):
    import d3p_amd._lib as L
    from d3p_amd import fidelity as F
    from d3p_amd import permutation as P
    m, d, R = 2 * T + 1, 3, 65
    z = grid_table(11, m, d, False)
    bits = _labels(np.random.default_rng(46), m, R)
    zt, lab = torch.tensor(z).cuda(), u32(PR.pack(bits))
    res = P.label_sums(zt, lab)                            # the default row sums: pair_stats(z, z, True)["sum"]
    t = F.pair_stats(zt, zt, True)["sum"]
    want = PR.restate(z, PR.pack(bits), np_(t))
    assert res.m == m and res.n1.dtype == torch.int64 and res.s11.dtype == torch.float64 and res.total.dim() == 0
    assert np.array_equal(np_(res.s11), want["s11"]) and np.array_equal(np_(res.s1t), want["s1t"]) and np.array_equal(np_(res.n1), want["n1"])
    assert float(res.total) == pytest.approx(float(np_(t).sum()), rel=1e-13)
    wide = torch.full((m, d + 5), 7.0, device="cuda")
    wide[:, :d] = zt
    strided = P.label_sums(wide[:, :d], lab, t)            # a row stride of its own
    assert torch.equal(WH.raw_bytes(strided.s11), WH.raw_bytes(res.s11))
    zi = torch.tensor(grid_table(12, m, d, True)).cuda()
    ints, floats = P.label_sums(zi, lab), P.label_sums(zi.float(), lab)      # int32 is converted when staged: the same table
    assert torch.equal(WH.raw_bytes(ints.s11), WH.raw_bytes(floats.s11)) and torch.equal(WH.raw_bytes(ints.s1t), WH.raw_bytes(floats.s1t))
    with pytest.raises(ValueError, match="beyond 2\\^24"):
        P.label_sums(torch.full((m, d), 2 ** 24 + 1, dtype=torch.int32, device="cuda"), lab)
    with pytest.raises(ValueError, match="different devices"):
        P.label_sums(zt, lab.cpu())
    with pytest.raises(ValueError, match="different devices"):
        P.label_sums(zt, lab, t.cpu())


def test_energy_test_on_the_device(LIB):
    from d3p_amd import fidelity as F
    from d3p_amd import permutation as P
    rng = np.random.default_rng(47)
    nx, ny, d, n_perm = S + 5, T + 3, 4, 130
    x, y = rng.normal(size=(nx, d)).astype(np.float32), (rng.normal(size=(ny, d)) + 0.3).astype(np.float32)
    xt, yt = torch.tensor(x).cuda(), torch.tensor(y).cuda()
    res = P.energy_test(xt, yt, n_perm=n_perm, seed=5)
    assert (res.n_perm, res.n_x, res.n_y, res.dim) == (n_perm, nx, ny, d) and res.d2.dtype == torch.float64
    m = nx + ny
    e = F.energy_distance(xt, yt)
    scale = 2 * float(e.exy) + float(e.exx) + float(e.eyy)
    assert abs(float(res.d2) - float(e.d2)) <= 8 * (m + PR.chain(m)) * 2.0 ** -53 * scale, (float(res.d2), float(e.d2))
    assert float(res.statistic) == pytest.approx(nx * ny / m * float(res.d2), rel=1e-14)
    # the count, BY VALUE: the restatement's arithmetic fed the device's sums
    zt = torch.cat([xt, yt])
    lab = P.permutation_labels(nx, ny, n_perm, seed=5, device="cuda")
    sums = P.label_sums(zt, lab)
    d2, stat = PR.statistics(np_(sums.s11), np_(sums.s1t), np_(sums.n1), float(sums.total), m)
    n_ge, p = PR.p_value(stat)
    assert (res.n_ge, res.p_value) == (n_ge, p) and res.p_value == (1 + res.n_ge) / (n_perm + 1)
    assert float(res.d2) == pytest.approx(d2[0], rel=1e-12) and float(res.null_mean) == pytest.approx(stat[1:].mean(), rel=1e-12)
    assert res.null_quantiles == pytest.approx(tuple(np.quantile(stat[1:], (0.5, 0.95, 0.99))), rel=1e-12)
    assert res.null_quantiles[0] <= res.null_quantiles[1] <= res.null_quantiles[2]
    # another seed: other relabellings, the same observed statistic, to the bit
    res2 = P.energy_test(xt, yt, n_perm=n_perm, seed=6)
    assert float(res2.statistic) == float(res.statistic) and res2.null_quantiles != res.null_quantiles
    # int32 tables; a 1-D table is d = 1
    xi, yi = torch.tensor(grid_table(13, 40, 2, True)).cuda(), torch.tensor(grid_table(14, 30, 2, True)).cuda()
    ri, rf = P.energy_test(xi, yi, n_perm=20), P.energy_test(xi.float(), yi.float(), n_perm=20)
    assert float(ri.statistic) == float(rf.statistic) and ri.p_value == rf.p_value
    assert P.energy_test(xt[:, 0], yt[:, 0], n_perm=9).dim == 1


def test_three_fixed_seed_cases(LIB):
    from d3p_amd import permutation as P
    x, y, n_perm = _fixed("equal")
    res = P.energy_test(torch.tensor(x).cuda(), torch.tensor(y).cuda(), n_perm=n_perm, seed=0)
    assert res.p_value == 1.0 and res.n_ge == n_perm and abs(float(res.statistic)) < 1e-12
    x, y, n_perm = _fixed("shifted")
    res = P.energy_test(torch.tensor(x).cuda(), torch.tensor(y).cuda(), n_perm=n_perm, seed=0)
    assert res.p_value == 1 / 200 and res.n_ge == 0 and float(res.statistic) > 5 * res.null_quantiles[2]
    x, y, n_perm = _fixed("independent")
    res = P.energy_test(torch.tensor(x).cuda(), torch.tensor(y).cuda(), n_perm=n_perm, seed=0)
    want = PR.energy_test(x, y, words(P.permutation_labels(45, 38, n_perm, seed=0)))
    assert 0.0 < res.p_value < 1.0 and (res.n_ge, res.p_value) == (want["n_ge"], want["p_value"])
    assert float(res.statistic) == pytest.approx(want["statistic"][0], rel=1e-9)


def test_more_labellings_than_one_call_takes(LIB, monkeypatch):
    """Above the kernel's cap energy_test walks chunks of labellings and reuses the row sums: the cap lowered to 64 changes nothing."""
    import d3p_amd._lib as L
    from d3p_amd import permutation as P
    x, y, _ = _fixed("independent")
    xt, yt = torch.tensor(x).cuda(), torch.tensor(y).cuda()
    whole = P.energy_test(xt, yt, n_perm=150, seed=2)
    lib = L.load()

    class Capped:
        def __getattr__(self, name):
            return (lambda: 64) if name == "d3p_pair_label_sums_max_labellings" else getattr(lib, name)
    monkeypatch.setattr(P._lib, "load", lambda: Capped())
    parts = P.energy_test(xt, yt, n_perm=150, seed=2)
    assert parts.n_ge == whole.n_ge and parts.p_value == whole.p_value and float(parts.statistic) == float(whole.statistic)
    assert parts.null_quantiles == whole.null_quantiles


def test_example_flag_reports_the_energy_test(gpu, capsys):
    spec = importlib.util.spec_from_file_location("ex_gmm_energy_test", os.path.join(ROOT, "examples", "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = dict(num_epochs=2, learning_rate=5e-2, batch_size=64, dimensions=2, num_samples=512, num_components=3, sigma=0.3,
                synthetic_fidelity=True)
    mod.main(argparse.Namespace(**base))
    old = [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("Epoch")]
    mod.main(argparse.Namespace(energy_test=49, **base))
    new = [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("Epoch")]
    added = [ln for ln in new if ln.startswith("energy distance permutation test")]
    assert len(added) == 1 and [ln for ln in new if ln is not added[0]] == old          # one line more, every other line unchanged
    m = re.search(r"\(49 relabellings\): to train statistic (-?[0-9.]+), p ([0-9.]+) \(null 95% ([0-9.]+)\); to test statistic (-?[0-9.]+), "
                  r"p ([0-9.]+) \(null 95% ([0-9.]+)\)", added[0])
    assert m
    for p in (float(m.group(2)), float(m.group(5))):
        assert 1 / 50 - 1e-4 <= p <= 1.0 and abs(p * 50 - round(p * 50)) < 0.01
    assert float(m.group(3)) > 0 and float(m.group(6)) > 0
    assert mod.parse_args(["--energy-test"]).energy_test == 199 and mod.parse_args(["--energy-test", "99"]).energy_test == 99
    assert mod.parse_args([]).energy_test is None
