"""d3p_amd.permutation without a GPU: the module surface and its lazy import, the declared symbols, the query functions, every refusal of
the C entry in the header's order and of the Python layer before the device is touched, permutation_labels, the source-text rules of
d3p_label_sums.hip, and the numpy restatement of the kernel's order (tests/permutation_ref.py) against the derived bound on
fidelity_ref's hostile cases and against cases solvable by hand."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import fidelity_ref as FR
from tests import permutation_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"d3p_pair_label_sums": 14, "d3p_pair_label_sums_tile_rows": 0, "d3p_pair_label_sums_block_labellings": 0,
         "d3p_pair_label_sums_max_labellings": 0, "d3p_pair_label_sums_workspace": 3}


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("permutation reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


def words(t):
    """A uint32 label tensor as a numpy uint32 array."""
    return t.cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ surface
def test_module_surface_and_declared_symbols():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import permutation as P
    assert d3p_amd.permutation is P and "permutation" in d3p_amd.__all__
    assert d3p_amd.__all__[-3:] == ["marginals", "fidelity", "energy"] and d3p_amd.__all__.index("permutation") < d3p_amd.__all__.index("marginals")
    assert P.__all__ == ["permutation_labels", "label_sums", "energy_test", "LabelSums", "EnergyTest", "INT_EXACT"]
    for name in ("permutation_labels", "label_sums", "energy_test"):
        assert callable(getattr(P, name))
    assert P.LabelSums._fields == ("s11", "s1t", "n1", "total", "m")
    assert P.EnergyTest._fields == ("d2", "statistic", "p_value", "n_perm", "null_mean", "null_quantiles", "n_ge", "n_x", "n_y", "dim")
    assert P.INT_EXACT == 2 ** 24
    for said in ("PRIVATE", "NOT covered by the accountant", "(1 + n_ge) / (n_perm + 1)", "TIE COUNTS", "DOES NOT SHOW", "too small to matter",
                 "HELD-OUT"):
        assert said in P.__doc__, said
    assert "not covered" in P.energy_test.__doc__
    hdr = open(os.path.join(ROOT, "include", "d3p_hip.h")).read()
    for name, n in ARITY.items():
        m = re.search(r"\b(?:int|uint32_t|size_t) " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).strip()
        assert (0 if args == "void" else args.count(",") + 1) == n == len(L.SIGNATURES[name][1]), name
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr) and "d3p_label_sums.hip; DESIGN.md 4y); added symbols, ABI 9" in hdr
    assert any(p.endswith("d3p_label_sums.hip") for p in L._SRC) and all(p in L._DEPS for p in L._SRC)
    lib = L.load()
    assert lib.d3p_abi_version() == 9 and all(hasattr(lib, name) for name in ARITY)
    for doc, pat in (("INTEGRATION.md", r"`d3p_pair_label_sums`"), ("README.md", r"d3p_amd\.permutation"), ("README.md", r"experiments_permutation\.md"),
                     ("DESIGN.md", r"4y\."), (os.path.join("docs", "experiments_permutation.md"), r"VGPR")):
        assert re.search(pat, open(os.path.join(ROOT, doc)).read()), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("4y."):]
    for said in ("4w", "half-walk", "matrix pipe", "MMD", "accountant", "bit for bit", "VGPR", "THE ORDER", "A = 32 + 32"):
        assert said in section, said


def test_import_stays_lazy():
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.permutation' not in sys.modules; " \
           "d3p_amd.permutation; assert 'd3p_amd.permutation' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_query_functions():
    import d3p_amd._lib as L
    lib = L.load()
    T, B, cap = lib.d3p_pair_label_sums_tile_rows(), lib.d3p_pair_label_sums_block_labellings(), lib.d3p_pair_label_sums_max_labellings()
    assert T == 32 == lib.d3p_pair_stats_tile_rows() and B % 64 == 0 and B >= 64 and cap >= 4096 and cap % B == 0
    assert T == PR.T
    for m, d, R in ((1, 1, 1), (2, 3, 1), (33, 2, 65), (4096, 2, 1000), (16384, 64, 1000), (4096, 784, 200), (2 ** 32 - 1, 1, cap)):
        assert lib.d3p_pair_label_sums_workspace(m, d, R) == 8 * R * -(-m // T), (m, d, R)       # one float64 per (tile, labelling)
    for bad in ((0, 4, 2), (4, 0, 2), (4, 4, 0), (4, 4, cap + 1)):
        assert lib.d3p_pair_label_sums_workspace(*bad) == 0


# ------------------------------------------------------------------------------------------------ the C entry's refusals
def test_the_c_entry_refuses_on_the_host_as_declared():
    """Everything the entry checks before it asks whether a pointer is device memory, in the header's order, and that question itself:
    the buffers here are host memory and are never reached."""
    import d3p_amd._lib as L
    lib = L.load()
    buf = np.zeros(8192, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    odd = C.c_void_p(buf.ctypes.data + 2)
    odd4 = C.c_void_p(buf.ctypes.data + 4)
    assert buf.ctypes.data % 8 == 0
    cap = lib.d3p_pair_label_sums_max_labellings()

    def run(z=p, dtype=0, ld=3, m=40, d=3, R=5, labels=p, row_sum=p, s11=p, s1t=p, n1=p, ws=p, ws_bytes=1 << 20):
        return lib.d3p_pair_label_sums(None, z, dtype, ld, m, d, R, labels, row_sum, s11, s1t, n1, ws, ws_bytes)
    need = lib.d3p_pair_label_sums_workspace(40, 3, 5)
    assert need == 2 * 5 * 8
    for name in ("z", "labels", "row_sum", "s11", "s1t", "n1", "ws"):
        assert run(**{name: None}) == -1 and b"null pointer" in lib.d3p_last_error(), name
    assert run(ws=None, m=0) == -1 and b"m >= 1" in lib.d3p_last_error()         # (no workspace at a refused shape: the shape is named)
    for name in ("z", "labels", "n1"):
        assert run(**{name: odd}) == -1 and b"not aligned to 4 bytes" in lib.d3p_last_error(), name
    for name in ("row_sum", "s11", "s1t", "ws"):
        assert run(**{name: odd4}) == -1 and b"not aligned to 8 bytes" in lib.d3p_last_error(), name
    assert run(z=None, labels=odd) == -1 and b"null pointer" in lib.d3p_last_error()                       # (the order: null before alignment)
    assert run(z=odd, dtype=7) == -1 and b"not aligned" in lib.d3p_last_error()                            # (alignment before dtype)
    for dtype in (-1, 2):
        assert run(dtype=dtype) == -1 and b"dtype must be 0 (float32) or 1 (int32)" in lib.d3p_last_error()
    assert run(dtype=3, m=0) == -1 and b"dtype" in lib.d3p_last_error()                                    # (dtype before m)
    assert run(m=0) == -1 and b"m >= 1" in lib.d3p_last_error()
    assert run(m=0, d=0, ld=0) == -1 and b"m >= 1" in lib.d3p_last_error()                                 # (m before d)
    assert run(d=0, ld=0) == -1 and b"d >= 1" in lib.d3p_last_error()
    for ld in (2, -1, 0):
        assert run(ld=ld) == -1 and b"ld >= d" in lib.d3p_last_error()
    assert run(ld=2 ** 62) == -1 and b"does not fit 63 bits" in lib.d3p_last_error()
    assert run(ld=2, R=0) == -1 and b"ld >= d" in lib.d3p_last_error()                                     # (ld before R)
    for R in (0, cap + 1, 2 ** 32 - 1):
        assert run(R=R) == -1 and b"labellings are required" in lib.d3p_last_error(), R
    big = 2 ** 32 - 1
    assert run(m=big, d=1, ld=1, R=cap, ws_bytes=0) == -3                                                  # (the grid before the workspace)
    msg = lib.d3p_last_error()
    assert b"2^31 - 1" in msg and str(-(-big // 32)).encode() in msg and str(cap // lib.d3p_pair_label_sums_block_labellings()).encode() in msg
    assert run(ws_bytes=need - 1) == -4 and b"workspace too small" in lib.d3p_last_error()
    assert run(ws_bytes=0) == -4 and b"workspace too small" in lib.d3p_last_error()
    for dtype in (0, 1):
        assert run(dtype=dtype, ws_bytes=need) == -1 and b"must be device memory" in lib.d3p_last_error()   # every value is fine
    assert run(R=cap, ws_bytes=2 ** 40) == -1 and b"must be device memory" in lib.d3p_last_error()
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ the Python layer's refusals
def test_python_layer_refuses_before_the_device(no_device):
    from d3p_amd import permutation as P
    z = torch.zeros((40, 3))
    lab = torch.zeros((2, 5), dtype=torch.int32).view(torch.uint32)
    for bad in (np.zeros((8, 3), np.float32), torch.zeros(()), z[None], z.double(), z.to(torch.int64), torch.zeros((0, 3)), torch.zeros((8, 0))):
        with pytest.raises(ValueError, match="a 2-D float32 or int32 CUDA tensor|at least one row|d >= 1"):
            P.label_sums(bad, lab)
        for args in ((bad, z), (z, bad)):
            with pytest.raises(ValueError, match="a 2-D float32 or int32 CUDA tensor|at least one row|d >= 1"):
                P.energy_test(*args)
    with pytest.raises(ValueError, match="unit stride"):
        P.label_sums(torch.zeros((3, 40)).t(), lab)
    with pytest.raises(ValueError, match="rows of the tensor overlap"):
        P.label_sums(torch.zeros((1, 3)).expand(40, 3), lab)
    for bad in (lab.view(torch.int32), lab.view(torch.int32).to(torch.int64), np.zeros((2, 5), np.uint32), lab[0], lab[None]):
        with pytest.raises(ValueError, match="labels: a 2-D uint32 tensor"):
            P.label_sums(z, bad)
    with pytest.raises(ValueError, match="40 rows of z need 2"):
        P.label_sums(z, torch.zeros((3, 5), dtype=torch.int32).view(torch.uint32))
    with pytest.raises(ValueError, match="at least one labelling"):
        P.label_sums(z, torch.zeros((2, 0), dtype=torch.int32).view(torch.uint32))
    with pytest.raises(ValueError, match="must be contiguous"):
        P.label_sums(z, torch.zeros((2, 10), dtype=torch.int32).view(torch.uint32)[:, ::2])
    import d3p_amd._lib as L
    cap = L.load().d3p_pair_label_sums_max_labellings()
    with pytest.raises(ValueError, match=f"at most {cap} in one call"):
        P.label_sums(z, torch.zeros((2, cap + 1), dtype=torch.int32).view(torch.uint32))
    for bad in (torch.zeros(40), torch.zeros(39, dtype=torch.float64), torch.zeros((40, 1), dtype=torch.float64), np.zeros(40),
                torch.zeros(80, dtype=torch.float64)[::2]):
        with pytest.raises(ValueError, match="row_sum: a contiguous float64 tensor"):
            P.label_sums(z, lab, row_sum=bad)
    with pytest.raises(ValueError, match="label_sums: z: .*CUDA tensor"):         # every value is fine; the tensors are the host's
        P.label_sums(z, lab, row_sum=torch.zeros(40, dtype=torch.float64))
    with pytest.raises(ValueError, match="one dtype for both"):
        P.energy_test(z, z.to(torch.int32))
    with pytest.raises(ValueError, match="one d for both"):
        P.energy_test(z, torch.zeros((5, 2)))
    for n_perm in (0, -1, 1.5, "9", True, None):
        with pytest.raises(ValueError, match="n_perm must be an int >= 1"):
            P.energy_test(z, z, n_perm=n_perm)
    for seed in (-1, 0.5, None):
        with pytest.raises(ValueError, match="seed must be an int >= 0"):
            P.energy_test(z, z, seed=seed)
    with pytest.raises(ValueError, match="energy_test: x: .*CUDA tensor"):
        P.energy_test(z, z)
    for args in ((0, 5, 9), (5, 0, 9), (5, 5, 0), (True, 5, 9), (5.0, 5, 9)):
        with pytest.raises(ValueError, match="must be an int >= 1"):
            P.permutation_labels(*args)
    with pytest.raises(ValueError, match="seed must be an int >= 0"):
        P.permutation_labels(5, 5, 9, seed=-3)


# ------------------------------------------------------------------------------------------------ permutation_labels
def test_permutation_labels():
    from d3p_amd import permutation as P
    for n_x, n_y, n_perm in ((1, 1, 3), (40, 56, 199), (31, 1, 7), (32, 32, 65), (5, 60, 130)):
        m = n_x + n_y
        lab = P.permutation_labels(n_x, n_y, n_perm, seed=3)
        assert lab.dtype == torch.uint32 and tuple(lab.shape) == (-(-m // 32), n_perm + 1) and lab.is_contiguous() and lab.device.type == "cpu"
        w = words(lab)
        bits = PR.unpack(w, m)
        assert np.array_equal(bits[0], np.arange(m) >= n_x)                                   # labelling 0: the identity
        assert (bits.sum(axis=1) == n_y).all()                                                # exactly n_y rows carry the 1
        assert np.array_equal(PR.pack(bits), w)                                               # (so: no bit at a row >= m)
        for chunk in (1, 7, 1000):
            assert torch.equal(P.permutation_labels(n_x, n_y, n_perm, seed=3, _chunk=chunk).view(torch.int32), lab.view(torch.int32)), chunk
        assert torch.equal(P.permutation_labels(n_x, n_y, n_perm, seed=3, device="cpu").view(torch.int32), lab.view(torch.int32))
        if m > 8:
            other = words(P.permutation_labels(n_x, n_y, n_perm, seed=4))
            assert np.array_equal(other[:, 0], w[:, 0]) and not np.array_equal(other, w)
            assert np.array_equal(words(P.permutation_labels(n_x, n_y, n_perm + 5, seed=3))[:, :n_perm + 1], w)     # a prefix: one draw per labelling
    # uniform over the subsets, roughly: every row of 8 carries the 1 in about half of 4000 labellings of 4 + 4
    freq = PR.unpack(words(P.permutation_labels(4, 4, 4000, seed=1)), 8)[1:].mean(axis=0)
    assert (np.abs(freq - 0.5) < 0.04).all(), freq


# ------------------------------------------------------------------------------------------------ the source's own rules
def test_source_text_rules():
    csrc = os.path.join(ROOT, "d3p_amd", "csrc")
    text = open(os.path.join(csrc, "d3p_label_sums.hip")).read()
    tile = open(os.path.join(csrc, "d3p_pair_tile.h")).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["d3p_device.h", "d3p_host.h", "d3p_pair_tile.h"]
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for banned in ("hipFuncSetAttribute", "147456", "? 0xffffffffu : 0x80000000u", "cdiv(*tiles,", "? cdiv(*", "row_workspace_check(",
                   ": the workspace must be", "threefry2x32(o0, o1, 0u, 0u", "1.0f / den", "d3p_colreduce.h", "d3p_row_sums.h"):
        assert banned not in text, banned
    for banned in ("atomic", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "mfma", "extern __shared__", "native", "fast"):
        assert banned not in code, banned
    header = text[:text.index("#include")]
    for said in ("THE RULE", "THE ORDER", "DETERMINISM", "fmaf chain", "2^24", "follow IEEE", "NaN or +-inf", "bit for bit", "IGNORED",
                 "never as an index", "J mod 4", "+0.0", "ascending I", "A = 32 + 32 ceil(tiles / 4) + 4 + tiles", "not on R", "inf - inf",
                 "No floating-point atomics", "no scratch", "no dynamic LDS", "D_ii is exactly +0.0"):
        assert said in header, said
    # the IEEE root, once; the tile's chain, not a restatement of it; the tile's constants, not copies
    assert code.count("sqrtf(") == 1 and "__builtin_sqrtf(q)" in code and "__fsqrt_rn" not in code
    assert "__fmaf_rn(" not in text and "pair_chain(va[ki], vb[kj], q[ki][kj])" in code
    assert not re.search(r"#define D3P_LS_(T|C|LD|WAVES)\b", text)
    num = {k: int(re.search(r"#define D3P_PAIR_" + k + r" (\d+)", tile).group(1)) for k in ("T", "C", "LD", "WAVES")}
    groups = int(re.search(r"#define D3P_LS_GROUPS (\d+)u", text).group(1))
    cap = int(re.search(r"#define D3P_LS_MAX_R (\d+)u", text).group(1))
    lds = num["T"] * num["LD"] * 4 * 2 * num["WAVES"] + num["T"] * num["T"] * 4 * num["WAVES"] + 4 * num["WAVES"]
    assert f"Static LDS: {lds} bytes" in header and lds < 64 * 1024
    assert 64 * groups * 8 == num["T"] * num["T"] * 4          # a slot's sums take exactly the place of its distances
    assert cap >= 4096 and cap % (64 * groups) == 0 and f"{64 * groups} consecutive labellings" in header
    hdr = open(os.path.join(ROOT, "include", "d3p_hip.h")).read()
    decl = hdr[hdr.index("Label sums of the pooled pair distances"):]
    for said in ("THE ORDER", "in this order", "D3P_E_UNSUPPORTED", "D3P_E_WORKSPACE", "ignored", f"= {cap}", "bit for bit", "+0.0"):
        assert said in decl, said


# ------------------------------------------------------------------------------------------------ the restatement
def _labels(rng, m, R):
    """R labellings of every density: none, all, one row, the identity split, and Bernoulli(p) for p over (0, 1)."""
    bits = np.zeros((R, m), bool)
    for r in range(R):
        kind = r % 6
        if kind == 1:
            bits[r] = True
        elif kind == 2:
            bits[r, rng.integers(m)] = True
        elif kind == 3:
            bits[r, m // 2:] = True
        elif kind > 3:
            bits[r] = rng.random(m) < rng.random()
    return bits


def _cases():
    rng = np.random.default_rng(17)
    yield "normal", rng.normal(size=(70, 5)).astype(np.float32)
    yield "clustered far from the origin", (1.0e4 + 1.0e-3 * rng.normal(size=(40, 2))).astype(np.float32)
    scale = (10.0 ** np.linspace(-6, 6, 13)).astype(np.float32)
    yield "columns over 12 decades", (rng.normal(size=(33, 13)) * scale).astype(np.float32)
    yield "0/1 at d = 784", rng.integers(0, 2, (15, 784)).astype(np.int32)
    yield "d = 1, two slots deep", rng.normal(size=PR.S + 3).astype(np.float32)


@pytest.mark.parametrize("name,z", list(_cases()), ids=[c[0] for c in _cases()])
def test_restatement_lies_within_the_derived_bound(name, z):
    rng = np.random.default_rng(5)
    m = z.shape[0]
    d = z.shape[1] if z.ndim == 2 else 1
    bits = _labels(rng, m, 13)
    lab = PR.pack(bits)
    t = PR.row_sums(z)
    got, ex = PR.restate(z, lab, t), PR.exact(z, lab)
    tol = PR.bound(ex, m, d)
    err = np.abs(got["s11"] - ex)
    assert (err <= tol).all(), (name, float((err[tol > 0] / tol[tol > 0]).max()))
    assert np.array_equal(got["n1"], bits.sum(axis=1))
    assert got["s11"][0] == 0.0 and got["s11"][2] == 0.0                   # no row, and one row: the diagonal is +0.0
    want = np.array([FR._fsum(t[b]) for b in bits])
    assert np.allclose(got["s1t"], want, rtol=(m + 2) * 2.0 ** -53, atol=0.0)
    assert abs(got["s11"][1] - FR._fsum(t)) <= (m + PR.chain(m) + 4) * 2.0 ** -53 * FR._fsum(t)     # all rows: the sum of the row sums
    print(f"{name}: largest error / bound {float((err[tol > 0] / tol[tol > 0]).max()):.3f}")


def test_chain_and_bound():
    assert PR.chain(2) == 32 + 32 + 4 + 1 and PR.chain(128) == 32 + 32 + 4 + 4 and PR.chain(129) == 32 + 64 + 4 + 5
    assert PR.chain(16384) == 32 + 32 * 128 + 4 + 512
    assert PR.bound(np.array([2.0]), 2, 2)[0] == (FR.rho(2) + 71 * 2.0 ** -53) * 2.0


def test_tail_bits_and_special_values_in_the_restatement():
    rng = np.random.default_rng(6)
    z = rng.normal(size=(37, 3)).astype(np.float32)
    bits = _labels(rng, 37, 7)
    lab = PR.pack(bits)
    t = PR.row_sums(z)
    base = PR.restate(z, lab, t)
    hostile = lab.copy()
    hostile[1] |= np.uint32((0xFFFFFFFF << (37 - 32)) & 0xFFFFFFFF)        # every bit of a row >= m set
    again = PR.restate(z, hostile, t)
    for k in ("s11", "s1t", "n1"):
        assert np.array_equal(base[k], again[k]), k
    for bad in (np.nan, np.inf, -np.inf):
        zz = z.copy()
        zz[20, 1] = bad
        out = PR.restate(zz, lab, t)
        assert np.isnan(out["s11"]).all() and np.array_equal(out["n1"], base["n1"]) and np.array_equal(out["s1t"], base["s1t"])
        assert np.isnan(PR.exact(zz, lab)).all()
    zz = z.copy()
    zz[5, 0] = 3e38                                                          # finite, q overflows: IEEE
    out = PR.restate(zz, lab, t)
    sel = bits[:, 5] & (bits.sum(axis=1) > 1)
    assert np.isinf(out["s11"][sel]).all() and np.isfinite(out["s11"][~sel]).all() and sel.any() and (~sel).any()


# ------------------------------------------------------------------------------------------------ by hand
def test_identities_on_nine_points_worked_by_hand():
    """x = 0, 1, 3, 7 and y = 2, 2, 5, 11, 12 on a line (d = 1), pooled z = [x; y], the identity labelling g = 0000 11111.
        S10 = sum_{y, x} |y - x| = (2+1+1+5) + (2+1+1+5) + (5+4+2+2) + (11+10+8+4) + (12+11+9+5) = 9 + 9 + 13 + 33 + 37 = 101
        s11 = sum over y x y = 2 (0 + 3 + 9 + 10 + 3 + 9 + 10 + 6 + 7 + 1) = 116
        S00 = sum over x x x = 2 (1 + 3 + 7 + 2 + 6 + 4) = 46
        t   = row sums of z: T = s11 + 2 S10 + S00 = 364,  s1t = s11 + S10 = 217
        d2  = 2 101 / 20 - 116 / 25 - 46 / 16 = 10.1 - 4.64 - 2.875 = 2.585,  statistic = 20 / 9 d2"""
    x, y = np.array([0, 1, 3, 7], np.int32), np.array([2, 2, 5, 11, 12], np.int32)
    z = np.concatenate([x, y])
    g = np.arange(9) >= 4
    rng = np.random.default_rng(2)
    bits = np.stack([g] + [rng.permutation(g) for _ in range(6)])
    lab = PR.pack(bits)
    t = PR.row_sums(z)
    assert t.sum() == 364.0
    out = PR.restate(z, lab, t)
    assert out["s11"][0] == 116.0 and out["s1t"][0] == 217.0 and out["n1"].tolist() == [5] * 7
    assert np.array_equal(out["s11"], PR.exact(z, lab))                                       # integers: every order agrees
    d2, stat = PR.statistics(out["s11"], out["s1t"], out["n1"], 364.0, 9)
    assert d2[0] == pytest.approx(2.585, rel=1e-15) and stat[0] == pytest.approx(20 / 9 * 2.585, rel=1e-15)
    D = np.abs(z[:, None].astype(np.float64) - z[None, :])
    for r in range(7):
        bd2, bstat = PR.brute(D, bits[r])
        assert d2[r] == pytest.approx(bd2, rel=1e-13, abs=1e-13) and stat[r] == pytest.approx(bstat, rel=1e-13, abs=1e-13)
    num, den, _ = FR.closed_form_d1(x, y)
    assert d2[0] == pytest.approx(num / den, rel=1e-14)
    # the torch arithmetic of the module is the same arithmetic
    from d3p_amd import permutation as P
    td2, tstat = P._statistics(torch.tensor(out["s11"]), torch.tensor(out["s1t"]), torch.tensor(out["n1"]), torch.tensor(364.0, dtype=torch.float64), 9)
    assert np.allclose(td2.numpy(), d2, rtol=1e-15, atol=0) and np.allclose(tstat.numpy(), stat, rtol=1e-15, atol=0)


def test_p_value_counts_ties():
    from d3p_amd import permutation as P
    for stat, n_ge, p in (([3, 1, 2, 3], 1, 2 / 4), ([0, 1, 1], 2, 1.0), ([5, 1, 2], 0, 1 / 3)):
        assert PR.p_value(stat) == (n_ge, p)
        assert P._p_value(torch.tensor(stat, dtype=torch.float64)) == (n_ge, p)


def _fixed(case):
    rng = np.random.default_rng(23)
    if case == "equal":
        x = rng.normal(size=(48, 3)).astype(np.float32)
        return x, x.copy(), 99
    if case == "shifted":
        return rng.normal(size=(40, 3)).astype(np.float32), (rng.normal(size=(56, 3)) + 3.0).astype(np.float32), 199
    return rng.normal(size=(45, 2)).astype(np.float32), rng.normal(size=(38, 2)).astype(np.float32), 99


def test_three_fixed_seed_cases_on_the_restatement():
    """The three cases of tests/test_gpu_permutation.py under permutation_labels' own labels: equal tables give p = 1, a shift of 3 the
    smallest p there is, two samples of one distribution something in between."""
    from d3p_amd import permutation as P
    x, y, n_perm = _fixed("equal")
    out = PR.energy_test(x, y, words(P.permutation_labels(48, 48, n_perm, seed=0)))
    assert out["p_value"] == 1.0 and abs(out["statistic"][0]) < 1e-12 and out["statistic"][1:].min() > 0.1
    x, y, n_perm = _fixed("shifted")
    out = PR.energy_test(x, y, words(P.permutation_labels(40, 56, n_perm, seed=0)))
    assert out["p_value"] == 1 / 200 and out["n_ge"] == 0 and out["statistic"][0] > 5 * out["statistic"][1:].max()
    x, y, n_perm = _fixed("independent")
    out = PR.energy_test(x, y, words(P.permutation_labels(45, 38, n_perm, seed=0)))
    assert 0 < out["n_ge"] < n_perm and 0.0 < out["p_value"] < 1.0
