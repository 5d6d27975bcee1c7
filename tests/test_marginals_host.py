"""d3p_amd.marginals without a GPU: the module surface and its lazy import, the declared symbols and query functions, every refusal of
the C entry in the header's order (on host buffers that are never reached) and of the Python layer before the device is touched, the
validation of caller-given edges, the source-text rules of d3p_marginals.hip, the numpy restatement (tests/marginals_ref.py) on cases
worked by hand, and the float64 summaries against rationals."""
import ctypes as C
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import marginals_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"d3p_marginals": 13, "d3p_marginals_max_bins": 0, "d3p_marginals_strip_rows": 0, "d3p_marginals_pair_tile": 0,
         "d3p_marginals_code_rows": 0, "d3p_marginals_workspace": 3}


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("marginals reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


# ------------------------------------------------------------------------------------------------ surface
def test_module_surface_and_declared_symbols():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import marginals as M
    names = d3p_amd.__all__
    assert d3p_amd.marginals is M and names.index("marginals") == names.index("fidelity") - 1 == len(names) - 3 and names[-1] == "energy"
    for name in ("bin_edges", "marginal_counts", "marginal_fidelity"):
        assert name in M.__all__ and callable(getattr(M, name))
    assert M.BinEdges._fields == ("edges", "nbins", "max_bins") and M.MarginalCounts._fields == ("one_way", "two_way", "pairs", "n")
    for f in ("tvd_one_way", "tvd_two_way", "tvd_one_way_mean", "tvd_two_way_mean", "worst_columns", "worst_pairs", "cramers_v_real",
              "cramers_v_synthetic", "assoc_diff_mean", "assoc_diff_max", "missing_real", "missing_synthetic", "floor"):
        assert f in M.MarginalFidelity._fields, f
    assert M.MAX_BINS == 32 and M.INT_EXACT == 2 ** 24
    assert "PRIVACY" in M.__doc__ and "PRIVATE" in M.__doc__ and "NOT covered by the accountant" in M.__doc__
    assert "not covered" in M.marginal_fidelity.__doc__ and "DEFINED as V = 0" in M.__doc__
    hdr = open(os.path.join(ROOT, "include", "d3p_hip.h")).read()
    for name, n in ARITY.items():
        m = re.search(r"\b(?:int|uint32_t|size_t) " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).strip()
        assert (0 if args == "void" else args.count(",") + 1) == n == len(L.SIGNATURES[name][1]), name
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr) and "d3p_marginals.hip; DESIGN.md 4x); added symbols,\n * ABI 9 unchanged" in hdr
    for said in ("searchsorted", "MISSING", "K = B + 1", "p = i (2 d - i - 1) / 2 + (j - i - 1)", "by construction", "zeroes both outputs"):
        assert said in hdr[hdr.index("d3p_marginals.hip"):], said
    assert any(p.endswith("d3p_marginals.hip") for p in L._SRC) and all(p in L._DEPS for p in L._SRC)
    lib = L.load()
    assert lib.d3p_abi_version() == 9 and all(hasattr(lib, name) for name in ARITY)
    for doc, pat in (("INTEGRATION.md", r"`d3p_marginals`"), ("README.md", r"d3p_amd\.marginals"), ("README.md", r"experiments_marginals\.md"),
                     ("DESIGN.md", r"4x\."), (os.path.join("docs", "experiments_marginals.md"), r"increments per second")):
        assert re.search(pat, open(os.path.join(ROOT, doc)).read()), doc


def test_import_stays_lazy():
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.marginals' not in sys.modules; " \
           "d3p_amd.marginals; assert 'd3p_amd.marginals' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_query_functions():
    import d3p_amd._lib as L
    lib = L.load()
    assert lib.d3p_marginals_max_bins() == 32
    S, Pt, R = lib.d3p_marginals_strip_rows(), lib.d3p_marginals_pair_tile(), lib.d3p_marginals_code_rows()
    assert S > 0 and Pt > 0 and R > 0
    assert S >= 8 * 33 * 33                       # the flush of K^2 cells per pair is small beside the strip's increments
    assert S < 2 ** 32                            # a 32-bit LDS counter cannot overflow within a strip
    for n, d, B in ((1, 1, 1), (2048, 2, 16), (10 ** 6, 64, 16), (4096, 784, 2), (2 ** 32 - 1, 3, 32)):
        assert lib.d3p_marginals_workspace(n, d, B) == n * d          # uint8 codes: at most n * d bytes
    for zero in ((0, 4, 2), (4, 0, 2), (4, 4, 0), (4, 4, 33)):
        assert lib.d3p_marginals_workspace(*zero) == 0


# ------------------------------------------------------------------------------------------------ the C entry's refusals
def test_the_c_entry_refuses_on_the_host_as_declared():
    """Everything the entry checks before it asks whether a pointer is device memory, in the header's order, and that question itself:
    the buffers here are host memory and are never reached."""
    import d3p_amd._lib as L
    lib = L.load()
    buf = np.zeros(8192, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    odd = C.c_void_p(buf.ctypes.data + 2)

    def run(x=p, dtype=0, ld=3, n=40, d=3, B=16, nb=p, e=p, one=p, two=p, ws=p, ws_bytes=1 << 20):
        return lib.d3p_marginals(None, x, dtype, ld, n, d, B, nb, e, one, two, ws, ws_bytes)
    for name in ("x", "nb", "e", "one", "two"):
        assert run(**{name: None}) == -1 and b"null pointer" in lib.d3p_last_error(), name
    for name in ("x", "nb", "e", "one", "two"):
        assert run(**{name: odd}) == -1 and b"not aligned to 4 bytes" in lib.d3p_last_error(), name
    for dtype in (-1, 2):
        assert run(dtype=dtype) == -1 and b"dtype must be 0 (float32) or 1 (int32)" in lib.d3p_last_error()
    assert run(n=0) == -1 and b"n >= 1" in lib.d3p_last_error()
    assert run(d=0, ld=0) == -1 and b"d >= 1" in lib.d3p_last_error()
    for ld in (2, -1, 0):
        assert run(ld=ld) == -1 and b"ld >= d" in lib.d3p_last_error()
    assert run(ld=2 ** 62) == -1 and b"does not fit 63 bits" in lib.d3p_last_error()
    for B in (0, 33, 2 ** 32 - 1):
        assert run(B=B) == -1 and b"1 <= B <= 32" in lib.d3p_last_error()
    assert run(x=None, ws_bytes=0, B=0, dtype=5) == -1 and b"null pointer" in lib.d3p_last_error()          # the order: null first
    assert run(x=odd, dtype=5) == -1 and b"not aligned" in lib.d3p_last_error()                            # alignment before dtype
    assert run(dtype=3, n=0) == -1 and b"dtype" in lib.d3p_last_error()                                     # dtype before n
    assert run(n=0, d=0, ld=0) == -1 and b"n >= 1" in lib.d3p_last_error()                                  # n before d
    assert run(ld=2, B=0) == -1 and b"ld >= d" in lib.d3p_last_error()                                      # ld before B
    assert run(B=0, ws_bytes=0) == -1 and b"1 <= B" in lib.d3p_last_error()                                 # B before the workspace
    assert run(ws_bytes=40 * 3 - 1) == -4 and b"workspace too small (119 < 120)" in lib.d3p_last_error()
    assert run(ws_bytes=0) == -4 and run(ws=None) == -4 and b"workspace too small" in lib.d3p_last_error()
    big = 2 ** 17 + 1                                   # 2^33 + 2^16 pairs: more pair tiles than a grid holds
    assert run(n=1, d=big, ld=big, ws_bytes=big) == -3 and b"2^31 - 1 workgroups" in lib.d3p_last_error() and b"d = 131073" in lib.d3p_last_error()
    assert run(n=1, d=big, ld=big, ws_bytes=big - 1) == -4                                                  # the workspace before the grid
    assert run(n=2 ** 32 - 1, d=400, ld=400, ws_bytes=2 ** 62) == -3 and b"workgroups" in lib.d3p_last_error()   # strips x tiles
    for dtype in (0, 1):
        assert run(dtype=dtype, ws_bytes=120) == -1 and b"must be device memory" in lib.d3p_last_error()   # every value is fine
    for B in (1, 32):
        assert run(B=B) == -1 and b"must be device memory" in lib.d3p_last_error()
    assert run(d=1, ld=1, two=None) == -1 and b"must be device memory" in lib.d3p_last_error()              # d = 1 has no pairs
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ the Python layer's refusals
def _edges(d, B=4):
    from d3p_amd import marginals as M
    return M.BinEdges(torch.zeros((d, max(B - 1, 1))), torch.ones(d, dtype=torch.int64), B)


def test_python_layer_refuses_before_the_device(no_device):
    from d3p_amd import marginals as M
    a, b = torch.zeros((8, 3)), torch.zeros((5, 3))
    pat = "a 2-D float32 or int32 CUDA tensor|at least one row|d >= 1"
    for bad in (np.zeros((8, 3), np.float32), torch.zeros(()), a[None], a.double(), a.to(torch.int64), torch.zeros((0, 3)), torch.zeros((8, 0))):
        with pytest.raises(ValueError, match=pat):
            M.bin_edges(bad)
        with pytest.raises(ValueError, match=pat):
            M.marginal_counts(bad, _edges(3))
        with pytest.raises(ValueError, match=pat):
            M.marginal_fidelity(bad, b)
        with pytest.raises(ValueError, match=pat):
            M.marginal_fidelity(a, bad)
        with pytest.raises(ValueError, match=pat):
            M.marginal_fidelity(a, b, holdout=bad)
    for fn in (lambda t: M.bin_edges(t), lambda t: M.marginal_counts(t, _edges(3)), lambda t: M.marginal_fidelity(t, b)):
        with pytest.raises(ValueError, match="unit stride"):
            fn(torch.zeros((3, 8)).t())
        with pytest.raises(ValueError, match="rows of the tensor overlap"):
            fn(torch.zeros((1, 3)).expand(8, 3))
        with pytest.raises(ValueError, match="CUDA tensor"):        # every value is fine; the tensor is the host's
            fn(a)
    # bin_edges
    for bins in (0, 33, -1, 2.5, True, "16", None):
        with pytest.raises(ValueError, match="bins must be an int in \\[1, 32\\]"):
            M.bin_edges(a, bins=bins)
        with pytest.raises(ValueError, match="bins must be an int in \\[1, 32\\]"):
            M.marginal_fidelity(a, b, bins=bins)
    for kind in ("quantiles", "", None, 3):
        with pytest.raises(ValueError, match="kind must be one of"):
            M.bin_edges(a, kind=kind)
        with pytest.raises(ValueError, match="kind must be one of"):
            M.marginal_fidelity(a, b, kind=kind)
    # marginal_counts
    for bad in (None, (torch.zeros((3, 3)), torch.ones(3, dtype=torch.int64), 4), "edges"):
        with pytest.raises(ValueError, match="a BinEdges"):
            M.marginal_counts(a, bad)
    with pytest.raises(ValueError, match="made for 2 columns, the table has 3"):
        M.marginal_counts(a, _edges(2))
    for B in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match="max_bins must be an int"):
            M.marginal_counts(a, M.BinEdges(torch.zeros((3, 3)), torch.ones(3, dtype=torch.int64), B))
    for e, nb in ((torch.zeros((3, 2)), torch.ones(3, dtype=torch.int64)), (torch.zeros((3, 3), dtype=torch.float64), torch.ones(3, dtype=torch.int64)),
                  (torch.zeros((3, 3)), torch.ones(3, dtype=torch.int32)), (torch.zeros(9), torch.ones(3, dtype=torch.int64)),
                  (np.zeros((3, 3), np.float32), torch.ones(3, dtype=torch.int64))):
        with pytest.raises(ValueError, match="CPU tensors edges"):
            M.marginal_counts(a, M.BinEdges(e, nb, 4))
    for nb in ([0, 1, 1], [1, 5, 1], [-1, 1, 1]):
        with pytest.raises(ValueError, match="nbins must lie in \\[1, 4\\]"):
            M.marginal_counts(a, M.BinEdges(torch.zeros((3, 3)), torch.tensor(nb), 4))
    for v in (float("nan"), float("inf"), float("-inf")):
        e = torch.zeros((3, 3))
        e[1, 1] = v
        with pytest.raises(ValueError, match="must be finite"):
            M.marginal_counts(a, M.BinEdges(e, torch.tensor([1, 3, 1]), 4))
        with pytest.raises(ValueError, match="CUDA tensor"):                        # an unused slot may hold anything
            M.marginal_counts(a, M.BinEdges(e, torch.tensor([4, 2, 4]), 4))
    e = torch.tensor([[0.0, 1.0, 0.5]] * 3)
    with pytest.raises(ValueError, match="non-decreasing"):
        M.marginal_counts(a, M.BinEdges(e, torch.tensor([1, 4, 1]), 4))
    with pytest.raises(ValueError, match="CUDA tensor"):
        M.marginal_counts(a, M.BinEdges(e, torch.tensor([1, 3, 1]), 4))
    wide = torch.zeros((4, 784))
    with pytest.raises(ValueError, match=f"{784 * 783 // 2} pair tables of 33 x 33 cells take {784 * 783 // 2 * 33 * 33 * 4} bytes, above max_bytes"):
        M.marginal_counts(wide, _edges(784, 32))
    with pytest.raises(ValueError, match="CUDA tensor"):
        M.marginal_counts(wide, _edges(784, 2))
    with pytest.raises(ValueError, match="take 48 bytes, above max_bytes = 47"):
        M.marginal_counts(a, _edges(3, 1), max_bytes=47)
    for mb in (-1, 1.5, None):
        with pytest.raises(ValueError, match="max_bytes must be"):
            M.marginal_counts(a, _edges(3), max_bytes=mb)
    # marginal_fidelity
    with pytest.raises(ValueError, match="one dtype for all"):
        M.marginal_fidelity(a, b.to(torch.int32))
    with pytest.raises(ValueError, match="one d for all"):
        M.marginal_fidelity(a, torch.zeros((5, 2)))
    with pytest.raises(ValueError, match="real has 3 columns and holdout has 1"):
        M.marginal_fidelity(a, b, holdout=torch.zeros(4))
    for cols in ([], [0, 0], [3], [-1], [0.0], [True], 2):
        with pytest.raises(ValueError, match="columns must be"):
            M.marginal_fidelity(a, b, columns=cols)
    for top in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match="top must be"):
            M.marginal_fidelity(a, b, top=top)
    with pytest.raises(ValueError, match="above max_bytes"):
        M.marginal_fidelity(torch.zeros((4, 784)), torch.zeros((4, 784)), bins=32)
    with pytest.raises(ValueError, match="list of 2 per-column edge sequences"):
        M.marginal_fidelity(a, b, bins=[[0.0]] * 3, columns=[0, 2])
    with pytest.raises(ValueError, match="CUDA tensor"):
        M.marginal_fidelity(a, b, bins=[[0.0], []], columns=[2, 0], holdout=b)


def test_caller_given_edges_are_validated_on_the_host(no_device):
    from d3p_amd import marginals as M
    a = torch.zeros((8, 3))                          # (a host tensor: caller-given edges never read the table)
    be = M.bin_edges(a, bins=[[0.0, 1.0, 1.0], [], np.array([-2.5], np.float32)])
    assert be.max_bins == 4 and be.nbins.tolist() == [4, 1, 2] and be.edges.shape == (3, 3) and be.edges.dtype == torch.float32
    assert be.edges.tolist() == [[0.0, 1.0, 1.0], [0.0, 0.0, 0.0], [-2.5, 0.0, 0.0]]
    one = M.bin_edges(a, bins=[[], [], []])
    assert one.max_bins == 1 and one.nbins.tolist() == [1, 1, 1] and one.edges.shape == (3, 1)
    full = M.bin_edges(a[:, :1], bins=[list(range(31))])
    assert full.max_bins == 32 and full.edges.shape == (1, 31)
    for v in (float("nan"), float("inf"), float("-inf"), 1e39):
        with pytest.raises(ValueError, match="finite"):
            M.bin_edges(a, bins=[[0.0, v], [], []])
    with pytest.raises(ValueError, match="column 1: the edges decrease at 2"):
        M.bin_edges(a, bins=[[], [0.0, 2.0, 1.0], []])
    with pytest.raises(ValueError, match="column 2: 32 edges; at most 31"):
        M.bin_edges(a, bins=[[], [], list(range(32))])
    with pytest.raises(ValueError, match="list of 3 per-column"):
        M.bin_edges(a, bins=[[0.0], [1.0]])
    with pytest.raises(ValueError, match="a sequence of numbers"):
        M.bin_edges(a, bins=[[0.0], "ab", []])
    with pytest.raises(ValueError, match="a sequence of numbers"):
        M.bin_edges(a, bins=[[0.0], 3, []])


# ------------------------------------------------------------------------------------------------ the source's own rules
def test_source_text_rules():
    csrc = os.path.join(ROOT, "d3p_amd", "csrc")
    text = open(os.path.join(csrc, "d3p_marginals.hip")).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["d3p_device.h", "d3p_host.h"]
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    for banned in ("hipFuncSetAttribute", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "mfma", "extern __shared__",
                   "double*", "unsafeAtomicAdd", "atomicCAS", "atomicMax", "atomicExch"):
        assert banned not in code, banned
    assert len(re.findall(r"atomicAdd\(", code)) == 4                 # two LDS increments, two flushes of non-zero cells
    assert len(re.findall(r"if \((?:v|s)\) atomicAdd\(a\.(?:one|two)_way", code)) == 2
    header = text[:text.index("#include")]
    for said in ("THE RULE", "SAFETY", "MISSING", "searchsorted", "right-closed", "-0.0 and 0.0 are equal", "K = B + 1", "BY CONSTRUCTION",
                 "p = i (2 d - i - 1) / 2 + (j - i - 1)", "zeroes both outputs", "replica", "none can overflow", "No scratch", "no dynamic LDS"):
        assert said in header, said
    num = {k: int(re.search(r"#define D3P_MG_" + k + r" (\d+)", text).group(1)) for k in ("MAX_BINS", "STRIP", "PT", "HIST_WORDS", "CODE_ROWS", "TC")}
    K = num["MAX_BINS"] + 1
    assert num["PT"] * K * K <= num["HIST_WORDS"] and num["HIST_WORDS"] * 4 < 64 * 1024          # static LDS stays below 64 KiB
    codes_lds = num["TC"] * (num["MAX_BINS"] - 1) * 4 + num["TC"] * 4 + num["TC"] * K * 4 + 4096 + num["TC"]
    assert f"Static LDS: {num['HIST_WORDS'] * 4} bytes (pairs), {codes_lds} bytes (codes)" in header
    import d3p_amd._lib as L
    lib = L.load()
    assert (lib.d3p_marginals_strip_rows(), lib.d3p_marginals_pair_tile(), lib.d3p_marginals_code_rows()) == (num["STRIP"], num["PT"], num["CODE_ROWS"])
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("4x."):]
    for said in ("searchsorted", "replica", "VGPR", "scratch", "Out of scope", "k-way", "accountant", "bincount"):
        assert said in section, said


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_reference_codes_on_cases_worked_by_hand():
    nan, inf = np.nan, np.inf
    # one column, B = 4, edges 1, 2, 2: bin 0 = (-inf, 1], bin 1 = (1, 2], bin 2 = (2, 2] is EMPTY (a duplicate edge), bin 3 = (2, inf)
    e = np.array([[1.0, 2.0, 2.0]], np.float32)
    x = np.array([-inf, 0.0, 1.0, 1.5, 2.0, np.nextafter(np.float32(2), np.float32(3)), 7.0, inf, nan], np.float32)
    assert MR.codes(x, e, [4], 4)[:, 0].tolist() == [0, 0, 0, 1, 1, 3, 3, 3, 4]
    one, two = MR.counts(x, e, [4], 4)
    assert one.tolist() == [[3, 2, 0, 3, 1]] and two.shape == (0, 5, 5)
    # the same edges with nb = 3: the third edge is not looked at
    assert MR.codes(x, e, [3], 4)[:, 0].tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 4]
    # nb = 1: one bin for every number, the missing cell for NaN
    assert MR.codes(x, e, [1], 4)[:, 0].tolist() == [0] * 8 + [4]
    # +-0 against an edge at 0 (either sign): equal, so bin 0
    for z in (0.0, -0.0):
        ez = np.array([[z]], np.float32)
        assert MR.codes(np.array([-0.0, 0.0, np.float32(1e-45), -np.float32(1e-45)], np.float32), ez, [2], 2)[:, 0].tolist() == [0, 0, 1, 0]
    # int32 values convert to float32
    assert MR.codes(np.array([-3, 0, 1, 2, 5], np.int32), np.array([[0.0, 1.0, 2.0]], np.float32), [4], 4)[:, 0].tolist() == [0, 0, 1, 2, 3]
    # two columns with their own nb, B = 3: a 2 x 2 x ... table by hand
    x2 = np.array([[0.0, 5.0], [1.0, 5.0], [1.0, nan], [3.0, -1.0], [nan, nan]], np.float32)
    e2 = np.array([[0.5, 2.0], [0.0, 99.0]], np.float32)
    assert MR.codes(x2, e2, [3, 2], 3).tolist() == [[0, 1], [1, 1], [1, 3], [2, 0], [3, 3]]
    one, two = MR.counts(x2, e2, [3, 2], 3)
    assert one.tolist() == [[1, 2, 1, 1], [1, 2, 0, 2]]
    want = np.zeros((4, 4), np.int64)
    want[0, 1] = want[1, 1] = want[1, 3] = want[2, 0] = want[3, 3] = 1
    assert two.shape == (1, 4, 4) and np.array_equal(two[0], want)
    assert np.array_equal(two[0].sum(axis=1), one[0]) and np.array_equal(two[0].sum(axis=0), one[1])


def test_the_two_restatements_of_the_counts_agree():
    rng = np.random.default_rng(11)
    for n, d, B in ((1, 1, 1), (7, 2, 3), (50, 5, 4), (33, 9, 32)):
        x = rng.normal(size=(n, d)).astype(np.float32)
        x[rng.random((n, d)) < 0.1] = np.nan
        nb = rng.integers(1, B + 1, d)
        e = np.sort(rng.normal(size=(d, max(B - 1, 1))).astype(np.float32), axis=1)
        (o1, t1), (o2, t2) = MR.counts(x, e, nb, B), MR.counts_product(x, e, nb, B)
        assert np.array_equal(o1, o2) and np.array_equal(t1, t2) and t1.shape == (d * (d - 1) // 2, B + 1, B + 1)
        assert (o1.sum(axis=1) == n).all() and (t1.sum(axis=(1, 2)) == n).all()


def test_reference_pair_index():
    assert [MR.pair_index(i, j, 2) for i, j in ((0, 1),)] == [0]
    assert [MR.pair_index(i, j, 3) for i, j in ((0, 1), (0, 2), (1, 2))] == [0, 1, 2]
    assert [MR.pair_index(i, j, 5) for i, j in ((0, 1), (0, 4), (1, 2), (1, 4), (2, 3), (2, 4), (3, 4))] == [0, 3, 4, 6, 7, 8, 9]
    for d in (2, 3, 5, 9):
        pr = MR.pairs(d)
        assert len(pr) == d * (d - 1) // 2 and all(MR.pair_index(i, j, d) == p for p, (i, j) in enumerate(pr))
        assert np.array_equal(pr, torch.triu_indices(d, d, 1).t().numpy())             # the order the Python layer reports
    assert MR.pairs(1).shape == (0, 2)


def test_summaries_against_rationals():
    from d3p_amd import marginals as M
    # one-way: counts (3, 1, 0, 1) over 5 rows against (2, 2, 4, 0) over 8: 1/2 (|3/5 - 1/4| + |1/5 - 1/4| + |0 - 1/2| + |1/5 - 0|)
    a, b = np.array([[3, 1, 0, 1]]), np.array([[2, 2, 4, 0]])
    want = Fraction(1, 2) * (abs(Fraction(3, 5) - Fraction(1, 4)) + abs(Fraction(1, 5) - Fraction(1, 4)) + Fraction(1, 2) + Fraction(1, 5))
    assert want == Fraction(11, 20)
    assert MR.tvd(a, 5, b, 8)[0] == pytest.approx(float(want), rel=1e-15)
    assert float(M._tvd(torch.tensor(a), 5, torch.tensor(b), 8)[0]) == pytest.approx(float(want), rel=1e-15)
    assert MR.tvd(a, 5, a, 5)[0] == 0.0 and float(M._tvd(torch.tensor(a), 5, torch.tensor(a), 5)[0]) == 0.0
    # Cramer's V of [[4, 0], [0, 4]] is 1 (chi^2 = n); of [[2, 2], [2, 2]] 0; of [[3, 1], [1, 3]] 1/2 (chi^2 = 4 x 1/2); the rest by rationals
    for tab, n in (([[4, 0, 0], [0, 4, 0], [0, 0, 0]], 8), ([[2, 2, 0], [2, 2, 0], [0, 0, 0]], 8), ([[3, 1, 0], [1, 3, 0], [0, 0, 0]], 8),
                   ([[5, 1, 2], [0, 3, 1], [2, 2, 4]], 20), ([[6, 0, 0], [2, 0, 0], [0, 0, 0]], 8), ([[0, 0, 0], [1, 2, 3], [0, 0, 0]], 6)):
        o = [[Fraction(v) for v in row] for row in tab]
        r = [sum(row) for row in o]
        c = [sum(o[u][v] for u in range(3)) for v in range(3)]
        k = min(sum(1 for v in r if v), sum(1 for v in c if v)) - 1
        if k < 1:
            want = 0.0                                   # DEFINED as 0: fewer than two non-empty rows or columns
        else:
            chi2 = sum((o[u][v] - r[u] * c[v] / n) ** 2 / (r[u] * c[v] / n) for u in range(3) for v in range(3) if r[u] * c[v])
            want = float(chi2 / (n * k)) ** 0.5
        assert MR.cramers_v(tab, n) == pytest.approx(want, rel=1e-14, abs=1e-300), tab
        assert float(M._cramers_v(torch.tensor([tab]), n)[0]) == pytest.approx(want, rel=1e-14, abs=1e-300), tab
    assert MR.cramers_v([[4, 0, 0], [0, 4, 0], [0, 0, 0]], 8) == 1.0 and MR.cramers_v([[2, 2, 0], [2, 2, 0], [0, 0, 0]], 8) == 0.0
    assert MR.cramers_v([[3, 1, 0], [1, 3, 0], [0, 0, 0]], 8) == pytest.approx(0.5, rel=1e-15)
    # the whole report from counts: _report against summaries on a small table
    rng = np.random.default_rng(5)
    xa, xb = rng.integers(0, 3, (40, 4)).astype(np.float32), rng.integers(0, 3, (25, 4)).astype(np.float32)
    xa[3, 1] = np.nan
    e = np.tile(np.array([[0.0, 1.0]], np.float32), (4, 1))
    (oa, ta), (ob, tb) = MR.counts(xa, e, [3] * 4, 3), MR.counts(xb, e, [3] * 4, 3)
    ref = MR.summaries(oa, ta, 40, ob, tb, 25)
    pr = torch.tensor(MR.pairs(4))
    be = M.BinEdges(torch.zeros((4, 2)), torch.full((4,), 3, dtype=torch.int64), 3)
    rep = M._report(M.MarginalCounts(torch.tensor(oa), torch.tensor(ta), pr, 40), M.MarginalCounts(torch.tensor(ob), torch.tensor(tb), pr, 25), 3, 2,
                    [7, 8, 9, 11], be)
    bound = 2 * (16 + 4) * 2.0 ** -53
    assert np.abs(rep.tvd_one_way.numpy() - ref["tvd_one_way"]).max() <= bound and np.abs(rep.tvd_two_way.numpy() - ref["tvd_two_way"]).max() <= bound
    assert np.allclose(rep.cramers_v_real.numpy(), ref["cramers_v_a"], rtol=1e-13, atol=0) and rep.assoc_diff_max == pytest.approx(ref["assoc_diff_max"], rel=1e-12)
    assert rep.missing_real.tolist() == [0.0, 1 / 40, 0.0, 0.0] and rep.missing_synthetic.tolist() == [0.0] * 4
    i = int(np.argmax(ref["tvd_two_way"]))
    assert len(rep.worst_pairs) == 2 and rep.worst_pairs[0][0] == tuple([7, 8, 9, 11][c] for c in MR.pairs(4)[i]) and rep.columns == (7, 8, 9, 11)
    assert rep.worst_columns[0][0] == [7, 8, 9, 11][int(np.argmax(ref["tvd_one_way"]))] and rep.floor is None
    assert rep.tvd_one_way_mean == pytest.approx(ref["tvd_one_way_mean"], rel=1e-14)


def test_quantile_rule_of_the_reference():
    # 10 values, 4 bins: ranks ceil(10 k / 4) - 1 = 2, 4, 7 -> the values there; the maximum is never an edge
    col = np.array([9, 1, 2, 3, 4, 5, 6, 7, 8, 0], np.float32)
    assert MR.quantile_edges(col, 4) == [2.0, 4.0, 7.0]
    assert MR.quantile_edges(np.array([0, 0, 0, 1, 1, 1, 1, 1], np.float32), 4) == [0.0]        # few distinct values: fewer bins
    assert MR.quantile_edges(np.array([5, 5, 5], np.float32), 16) == [] and MR.quantile_edges(np.array([np.nan, np.inf]), 4) == []
    assert MR.quantile_edges(np.array([1, np.nan, 3, -np.inf, 2, np.inf], np.float32), 3) == [1.0, 2.0]
