"""d3p_amd.fidelity without a GPU: the module surface and its lazy import, the declared symbols, the query functions and the form aid,
every refusal of the C entry and of the Python layer before the device is touched, the source-text rules of d3p_pair_stats.hip, and the
numpy emulation of the kernel's rule (tests/fidelity_ref.py) against the derived bound -- including rows clustered far from the origin,
the case a Gram-matrix distance would lose -- and against cases solvable by hand."""
import ctypes as C
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import fidelity_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"d3p_pair_stats": 15, "d3p_pair_stats_tile_rows": 0, "d3p_pair_stats_chunk_cols": 0, "d3p_pair_stats_segment_tiles": 0,
         "d3p_pair_stats_form": 3, "d3p_pair_stats_workspace": 3, "d3p_pair_stats_set_form": 1}


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("fidelity reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


# ------------------------------------------------------------------------------------------------ surface
def test_module_surface_and_declared_symbols():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import fidelity as F
    assert d3p_amd.fidelity is F and "fidelity" in d3p_amd.__all__ and d3p_amd.__all__.index("fidelity") == len(d3p_amd.__all__) - 2
    for name in ("pair_stats", "energy_distance", "closest_record", "fidelity_report"):
        assert name in F.__all__ and callable(getattr(F, name))
    assert F.EnergyDistance._fields == ("d2", "d2_unbiased", "exy", "exx", "eyy", "n_x", "n_y", "dim")
    assert F.FidelityReport._fields == ("energy_train", "energy_holdout", "dcr_probs", "dcr_quantiles", "n_exact_copies", "aa_truth", "aa_synth",
                                        "aa", "aa_holdout", "privacy_loss", "closer_to_train", "n_train", "n_synthetic", "n_holdout", "dim")
    assert F.INT_EXACT == 2 ** 24 and "PRIVATE" in F.__doc__ and "not covered" in F.fidelity_report.__doc__
    hdr = open(os.path.join(ROOT, "include", "d3p_hip.h")).read()
    for name, n in ARITY.items():
        m = re.search(r"\b(?:int|uint32_t|size_t) " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).strip()
        assert (0 if args == "void" else args.count(",") + 1) == n == len(L.SIGNATURES[name][1]), name
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr) and "d3p_pair_stats.hip; DESIGN.md 4w); added symbols, ABI 9 unchanged" in hdr
    assert any(p.endswith("d3p_pair_stats.hip") for p in L._SRC) and all(p in L._DEPS for p in L._SRC)
    lib = L.load()
    assert lib.d3p_abi_version() == 9 and all(hasattr(lib, name) for name in ARITY)
    for doc, pat in (("INTEGRATION.md", r"`d3p_pair_stats`"), ("README.md", r"d3p_amd\.fidelity"), ("DESIGN.md", r"4w\."),
                     (os.path.join("docs", "experiments_fidelity.md"), r"error / bound")):
        assert re.search(pat, open(os.path.join(ROOT, doc)).read()), doc


def test_import_stays_lazy():
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.fidelity' not in sys.modules; " \
           "d3p_amd.fidelity; assert 'd3p_amd.fidelity' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_query_functions_and_the_form_aid():
    import d3p_amd._lib as L
    lib = L.load()
    T, Cc, G = lib.d3p_pair_stats_tile_rows(), lib.d3p_pair_stats_chunk_cols(), lib.d3p_pair_stats_segment_tiles()
    assert T >= 8 and Cc >= 4 and Cc % 4 == 0 and G >= 4 and G % 4 == 0           # (a segment holds every slot equally often)
    seg = G * T
    try:
        assert lib.d3p_pair_stats_set_form(0) == 0
        for na, nb, d in ((1, 1, 1), (2048, 2048, 2), (8192, 8192, 64), (4096, 4096, 784), (65536, 65536, 64), (2 ** 32 - 1, 7, 3)):
            assert lib.d3p_pair_stats_form(na, nb, d) in (1, 2), (na, nb, d)
        assert lib.d3p_pair_stats_form(2048, 2048, 2) == 2            # 64 tiles of a cannot fill the chip: the segments are dealt out
        assert lib.d3p_pair_stats_form(10 ** 6, 10 ** 6, 64) == 1     # the tiles of a alone fill it: no workspace
        assert lib.d3p_pair_stats_form(2048, seg, 2) == 1             # one segment: nothing to deal out
        assert lib.d3p_pair_stats_form(2048, seg + 1, 2) == 2
        for zero in ((0, 4, 2), (4, 0, 2), (4, 4, 0)):
            assert lib.d3p_pair_stats_form(*zero) == 0 and lib.d3p_pair_stats_workspace(*zero) == 0
        assert lib.d3p_pair_stats_workspace(10 ** 6, 10 ** 6, 64) == 0
        assert lib.d3p_pair_stats_workspace(2048, seg + 1, 2) == 2 * 2048 * 20     # a double, a packed minimum and a flag word per cell
        for form in (1, 2):
            assert lib.d3p_pair_stats_set_form(form) == 0
            assert lib.d3p_pair_stats_form(2048, 2048, 2) == form and lib.d3p_pair_stats_form(10 ** 6, 10 ** 6, 64) == form
        assert lib.d3p_pair_stats_workspace(5, 3, 1) == 1 * 5 * 20     # (the forced split form at one segment)
        assert lib.d3p_pair_stats_set_form(1) == 0 and lib.d3p_pair_stats_workspace(2048, 2048, 2) == 0
        for form in (-1, 3, 7):
            assert lib.d3p_pair_stats_set_form(form) == -1 and b"form must be" in lib.d3p_last_error()
    finally:
        assert lib.d3p_pair_stats_set_form(0) == 0


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

    def run(a=p, b=p, dtype=0, a_ld=3, b_ld=3, na=40, nb=1000, d=3, excl=0, s=p, m=p, am=p, ws=p, ws_bytes=1 << 20):
        return lib.d3p_pair_stats(None, a, b, dtype, a_ld, b_ld, na, nb, d, excl, s, m, am, ws, ws_bytes)
    try:
        assert lib.d3p_pair_stats_set_form(2) == 0
        need = lib.d3p_pair_stats_workspace(40, 1000, 3)
        assert need == -(-1000 // (lib.d3p_pair_stats_tile_rows() * lib.d3p_pair_stats_segment_tiles())) * 40 * 20
        for name in ("a", "b", "s", "m", "am"):
            assert run(**{name: None}) == -1 and b"null pointer" in lib.d3p_last_error(), name
        for name in ("a", "b", "m", "am"):
            assert run(**{name: odd}) == -1 and b"not aligned to 4 bytes" in lib.d3p_last_error(), name
        for name in ("s", "ws"):
            assert run(**{name: odd4}) == -1 and b"not aligned to 8 bytes" in lib.d3p_last_error(), name
        for dtype in (-1, 2):
            assert run(dtype=dtype) == -1 and b"dtype must be 0 (float32) or 1 (int32)" in lib.d3p_last_error()
        assert run(na=0) == -1 and b"na >= 1 and nb >= 1" in lib.d3p_last_error()
        assert run(nb=0) == -1 and b"na >= 1 and nb >= 1" in lib.d3p_last_error()
        assert run(d=0, a_ld=0, b_ld=0) == -1 and b"d >= 1" in lib.d3p_last_error()
        for ld in (2, -1, 0):
            assert run(a_ld=ld) == -1 and b"a_ld >= d" in lib.d3p_last_error()
            assert run(b_ld=ld) == -1 and b"b_ld >= d" in lib.d3p_last_error()
        assert run(a_ld=2 ** 62) == -1 and b"does not fit 63 bits" in lib.d3p_last_error()
        for excl in (-1, 2):
            assert run(excl=excl, nb=40) == -1 and b"exclude_diagonal must be 0 or 1" in lib.d3p_last_error()
        assert run(excl=1) == -1 and b"na == nb is required" in lib.d3p_last_error()
        assert run(dtype=3, na=0, ws_bytes=0) == -1 and b"dtype" in lib.d3p_last_error()                     # (the order: dtype before na)
        assert run(excl=1, ws_bytes=0) == -1 and b"na == nb" in lib.d3p_last_error()                         # (the flag before the workspace)
        assert run(ws_bytes=need - 1) == -4 and b"workspace too small" in lib.d3p_last_error()
        assert run(ws_bytes=0) == -4 and run(ws=None) == -4 and b"workspace too small" in lib.d3p_last_error()
        big = 2 ** 32 - 1
        assert run(na=big, nb=big, d=1, a_ld=1, b_ld=1, ws_bytes=2 ** 62) == -3 and b"2^31 - 1 workgroups" in lib.d3p_last_error()
        assert run(na=big, nb=big, d=1, a_ld=1, b_ld=1, ws_bytes=2 ** 40) == -4                              # (the workspace before the grid)
        for dtype in (0, 1):
            assert run(dtype=dtype, ws_bytes=need) == -1 and b"must be device memory" in lib.d3p_last_error()   # every value is fine
        assert run(excl=1, nb=40) == -1 and b"must be device memory" in lib.d3p_last_error()
        assert lib.d3p_pair_stats_set_form(1) == 0
        assert run(ws=None, ws_bytes=0) == -1 and b"must be device memory" in lib.d3p_last_error()           # the wide form needs none
        assert run(na=big, nb=big, d=1, a_ld=1, b_ld=1, ws=None, ws_bytes=0) == -1 and b"must be device memory" in lib.d3p_last_error()
    finally:
        assert lib.d3p_pair_stats_set_form(0) == 0
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ the Python layer's refusals
def test_python_layer_refuses_before_the_device(no_device):
    from d3p_amd import fidelity as F
    a, b = torch.zeros((8, 3)), torch.zeros((5, 3))
    two = {"pair_stats": F.pair_stats, "energy_distance": F.energy_distance, "closest_record": F.closest_record,
           "fidelity_report": F.fidelity_report}
    for name, fn in two.items():
        for bad in (np.zeros((8, 3), np.float32), torch.zeros(()), a[None], a.double(), a.to(torch.int64), torch.zeros((0, 3)),
                    torch.zeros((8, 0))):
            with pytest.raises(ValueError, match="a 2-D float32 or int32 CUDA tensor|at least one row|d >= 1"):
                fn(bad, b)
            with pytest.raises(ValueError, match="a 2-D float32 or int32 CUDA tensor|at least one row|d >= 1"):
                fn(b, bad)
        with pytest.raises(ValueError, match="unit stride"):
            fn(torch.zeros((3, 8)).t(), b)
        with pytest.raises(ValueError, match="rows of the tensor overlap"):
            fn(torch.zeros((1, 3)).expand(8, 3), b)
        with pytest.raises(ValueError, match="one dtype for both"):
            fn(a, b.to(torch.int32))
        with pytest.raises(ValueError, match="one d for both"):
            fn(a, torch.zeros((5, 2)))
        with pytest.raises(ValueError, match="one d for both"):
            fn(a, torch.zeros(5))                                        # (the 1-D form is d = 1)
        with pytest.raises(ValueError, match=f"{name}: .*CUDA tensor"):  # every value is fine; the tensors are the host's
            fn(a, b)
        with pytest.raises(ValueError, match="CUDA tensor"):
            fn(torch.zeros(8, dtype=torch.int32), torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match="8 rows against 5"):
        F.pair_stats(a, b, exclude_diagonal=True)
    for flag in (2, "yes", None, 0.5):
        with pytest.raises(ValueError, match="exclude_diagonal must be a bool"):
            F.pair_stats(a, a, exclude_diagonal=flag)
    with pytest.raises(ValueError, match="CUDA tensor"):
        F.pair_stats(a, a, exclude_diagonal=True)
    with pytest.raises(ValueError, match="one d for both"):
        F.fidelity_report(a, b, holdout=torch.zeros((4, 2)))
    with pytest.raises(ValueError, match="one dtype for both"):
        F.fidelity_report(a, b, holdout=torch.zeros((4, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="holdout: a 2-D float32"):
        F.fidelity_report(a, b, holdout=np.zeros((4, 3), np.float32))
    for probs in ((1.5,), (-0.1, 0.5), (float("nan"),), 0.5, tuple([0.5] * 9)):
        with pytest.raises(ValueError, match="probs"):
            F.fidelity_report(a, b, probs=probs)
    with pytest.raises(ValueError, match="CUDA tensor"):
        F.fidelity_report(a, b, holdout=torch.zeros((4, 3)))


# ------------------------------------------------------------------------------------------------ the source's own rules
def test_source_text_rules():
    csrc = os.path.join(ROOT, "d3p_amd", "csrc")
    text = open(os.path.join(csrc, "d3p_pair_stats.hip")).read()
    tile = open(os.path.join(csrc, "d3p_pair_tile.h")).read()          # the 32 x 32 pair tile, shared with d3p_energy.hip
    assert re.findall(r'#include "([^"]+)"', text) == ["d3p_device.h", "d3p_host.h", "d3p_pair_tile.h"]
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    tile_code = "\n".join(line.split("//")[0] for line in tile.splitlines())
    for banned in ("hipFuncSetAttribute", "147456", "atomic", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "mfma",
                   "extern __shared__", "d3p_row_sums.h", "d3p_colreduce.h"):
        assert banned not in code and banned not in tile_code, banned
    header = text[:text.index("#include")]
    for said in ("THE RULE", "THE ORDER", "DETERMINISM", "fmaf chain", "2^24", "follow IEEE", "NaN or +-inf", "bit for bit", "Gram matrix",
                 "SMALLEST j", "(bits(q) << 32) | j", "0xFFFFFFFF", "J mod 4", "butterfly 4, 2, 1", "ascending segment order", "exclude_diagonal",
                 "not on na", "the form"):
        assert said in header, said
    # the IEEE root: this toolchain's __fsqrt_rn is the native instruction (1 ulp) unless OCML_BASIC_ROUNDED_OPERATIONS is defined
    assert code.count("sqrtf(") == 1 and "__builtin_sqrtf(q)" in code and "__fsqrt_rn" not in code and "sqrt" not in tile_code
    assert "native" not in code and "fast" not in code and "native" not in tile_code and "fast" not in tile_code
    num = {k: int(re.search(r"#define D3P_PAIR_" + k + r" (\d+)", tile).group(1)) for k in ("T", "C", "LD", "WAVES")}
    num["G"] = int(re.search(r"#define D3P_PS_G (\d+)", text).group(1))
    lds = num["T"] * num["LD"] * 4 * 2 * num["WAVES"] + num["T"] * num["WAVES"] * (2 * 8 + 8 + 4) + 4 * num["WAVES"]
    assert f"Static LDS: {lds} bytes" in header and lds < 64 * 1024          # static LDS stays below 64 KiB
    assert num["G"] % num["WAVES"] == 0 and num["LD"] % 4 == 0 and num["LD"] >= num["C"]
    # the distance of d3p_energy.hip: ONE chain, the tile's, columns x, y, z, w ascending; neither file restates it or the constants
    energy = open(os.path.join(csrc, "d3p_energy.hip")).read()
    chain = r"float tt = va\.x - vb\.x; q = __fmaf_rn\(tt, tt, q\); tt = va\.y - vb\.y; q = __fmaf_rn\(tt, tt, q\); " \
            r"tt = va\.z - vb\.z; q = __fmaf_rn\(tt, tt, q\); tt = va\.w - vb\.w; return __fmaf_rn\(tt, tt, q\);"
    assert len(re.findall(chain, re.sub(r"\s+", " ", tile_code))) == 1 and tile_code.count("__fmaf_rn(") == 4
    for name, src in (("d3p_pair_stats.hip", text), ("d3p_energy.hip", energy)):
        assert "__fmaf_rn(" not in src and "pair_chain(va[ki], vb[kj], q[ki][kj])" in src, name
        assert not re.search(r"#define D3P_(ES|PS)_(T|C|LD|WAVES)\b", src), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("4w."):]
    for said in ("Gram", "permutation", "half-walk", "MMD", "categorical", "VGPR", "bit for bit", "d3p_energy.hip", "accountant"):
        assert said in section, said


# ------------------------------------------------------------------------------------------------ the restatement
def _cases():
    rng = np.random.default_rng(17)
    yield "normal", rng.normal(size=(37, 5)).astype(np.float32), rng.normal(size=(70, 5)).astype(np.float32), False
    far = (1.0e4 + 1.0e-3 * rng.normal(size=(40, 2))).astype(np.float32)
    yield "clustered far from the origin", far, far, True
    scale = (10.0 ** np.linspace(-6, 6, 13)).astype(np.float32)
    yield "columns over 12 decades", (rng.normal(size=(20, 13)) * scale).astype(np.float32), (rng.normal(size=(33, 13)) * scale).astype(np.float32), False
    yield "0/1 at d = 784", rng.integers(0, 2, (6, 784)).astype(np.int32), rng.integers(0, 2, (9, 784)).astype(np.int32), False
    yield "d = 1", rng.normal(size=17).astype(np.float32), rng.normal(size=6).astype(np.float32), False


@pytest.mark.parametrize("name,a,b,excl", list(_cases()), ids=[c[0] for c in _cases()])
def test_emulation_lies_within_the_derived_bound(name, a, b, excl):
    d = a.shape[1] if a.ndim == 2 else 1
    nb = b.shape[0]
    ex, em = FR.exact(a, b, excl), FR.emulate(a, b, excl)
    tol = FR.bound(ex, nb, d)
    worst = 0.0
    for k in ("sum", "min"):
        err = np.abs(em[k].astype(np.float64) - ex[k])
        assert (err <= tol[k]).all(), (name, k, float((err / tol[k]).max()))
        worst = max(worst, float((err[tol[k] > 0] / tol[k][tol[k] > 0]).max()))
    rows = np.arange(a.shape[0])
    assert (ex["dist"][rows, em["argmin"]] <= ex["min"] * (1.0 + 2.0 * FR.rho(d))).all()       # the index by property
    assert not excl or (em["argmin"] != rows).all()
    print(f"{name}: largest error / bound {worst:.3f}")
    if name == "clustered far from the origin":
        # what the rule is for: a Gram-matrix distance |a|^2 + |b|^2 - 2 a.b in float32 loses these distances entirely
        z = a.astype(np.float32)
        sq = (z * z).sum(axis=1, dtype=np.float32)
        gram = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - np.float32(2) * (z @ z.T), 0)).astype(np.float64)
        np.fill_diagonal(gram, np.inf)
        assert (np.abs(gram.min(axis=1) - ex["min"]) > 100 * tol["min"]).any()


def test_restatement_on_cases_solvable_by_hand():
    # d = 1, integer points: a = 0, 4, 9 against b = 1, 4, 4, 10 -- sums 1+4+4+10, 3+0+0+6, 8+5+5+1; the nearest of 4 is the FIRST 4
    a, b = np.array([0, 4, 9], np.int32), np.array([1, 4, 4, 10], np.int32)
    for f in (FR.exact, FR.emulate):
        out = f(a, b)
        assert out["sum"].tolist() == [19.0, 9.0, 19.0] and out["min"].tolist() == [1.0, 0.0, 1.0] and out["argmin"].tolist() == [0, 1, 3]
    # a table against itself without the diagonal: 0, 4, 9 -> sums 13, 9, 14, nearest 4, 4, 5; one row alone has no pair
    out = FR.emulate(a, a, True)
    assert out["sum"].tolist() == [13.0, 9.0, 14.0] and out["min"].tolist() == [4.0, 4.0, 5.0] and out["argmin"].tolist() == [1, 0, 1]
    out = FR.emulate(a[:1], a[:1], True)
    assert out["sum"][0] == 0.0 and out["min"][0] == np.inf and out["argmin"][0] == -1
    # d = 2, points k (3, 4): every distance is 5 |k_i - k_j|
    ka, kb = np.array([0, 2, -1, 5], np.float32), np.array([1, 7, -3], np.float32)
    out = FR.emulate(ka[:, None] * np.array([3, 4], np.float32), kb[:, None] * np.array([3, 4], np.float32))
    want = 5.0 * np.abs(ka[:, None].astype(np.float64) - kb[None, :])
    assert np.array_equal(out["sum"], want.sum(axis=1)) and np.array_equal(out["min"], want.min(axis=1).astype(np.float32))
    assert out["argmin"].tolist() == [0, 0, 0, 1]                      # (-1 lies 10 from both 1 and -3: the first)
    # two equal tables: the diagonal's zero adds nothing, so the three walks give equal sums and d2 == 0 exactly
    x = np.random.default_rng(3).normal(size=(9, 4)).astype(np.float32)
    xy, xx = FR.emulate(x, x), FR.emulate(x, x, True)
    assert np.array_equal(xy["sum"], xx["sum"])
    d2, d2u, exy, exx, eyy = FR.energy(xy["sum"], xx["sum"], xx["sum"], 9, 9)
    assert d2 == 0.0 and exy == exx == eyy and d2u < 0                  # (the unbiased form removes the diagonal's share)
    # d = 1 in exact integers
    xs, ys = np.array([0, 1, 3, 7], np.int32), np.array([2, 2, 5], np.int32)
    num, den, (sxy, sxx, syy) = FR.closed_form_d1(xs, ys)
    assert (sxy, sxx, syy) == (31, 46, 12) and Fraction(num, den) == Fraction(2 * 31, 12) - Fraction(46, 16) - Fraction(12, 9)
    got = FR.energy(FR.emulate(xs, ys)["sum"], FR.emulate(xs, xs, True)["sum"], FR.emulate(ys, ys, True)["sum"], 4, 3)
    assert got[0] == pytest.approx(num / den, rel=1e-15) and got[1] == pytest.approx(2 * 31 / 12 - 46 / 12 - 12 / 6, rel=1e-14)
    assert np.isnan(FR.energy(np.zeros(1), np.zeros(1), np.zeros(3), 1, 3)[1])                  # one row: 0 / 0
    # special values: NaN by row of a, a NaN in b for every row; overflow of q follows IEEE
    a = np.zeros((3, 2), np.float32)
    b = np.zeros((4, 2), np.float32)
    a[1, 0] = np.nan
    a[2, 1] = 1e30
    out = FR.emulate(a, b)
    assert out["sum"][0] == 0.0 and np.isnan(out["sum"][1]) and np.isnan(out["min"][1]) and out["argmin"][1] == -1
    assert out["sum"][2] == np.inf and out["min"][2] == np.inf and out["argmin"][2] == 0        # ties at inf: the smallest j
    assert np.isfinite(FR.exact(a, b)["sum"][2])
    b[3, 1] = -np.inf
    out = FR.emulate(a, b)
    assert np.isnan(out["sum"]).all() and np.isnan(out["min"]).all() and (out["argmin"] == -1).all()


def test_report_on_six_points_worked_out_by_hand():
    """T = 0, 1, 3 and S = 0, 8, 12 on a line (d = 1).
        d_TT = 1, 1, 2      d_TS = 0, 1, 3      1[d_TS > d_TT] = 0, 0, 1      aa_truth = 1/3
        d_SS = 8, 4, 4      d_ST = 0, 5, 9      1[d_ST > d_SS] = 0, 1, 1      aa_synth = 2/3      aa = 1/2      one exact copy (0)
    With the holdout H = 2, 13, 20:
        d_HH = 11, 7, 7     d_HS = 2, 1, 8      1[d_HS > d_HH] = 0, 0, 1      -> 1/3
        d_SH = 2, 5, 1                          1[d_SH > d_SS] = 0, 1, 0      -> 1/3      aa_holdout = 1/3      privacy loss = -1/6
        d_ST < d_SH: yes, a tie (5 = 5), no                                   closer_to_train = (1 + 1/2 + 0) / 3 = 1/2
    The quantiles of d_ST = 0, 5, 9 at 0, 1/2, 1 are 0, 5, 9; at 1/4: 2.5."""
    T, S, H = np.array([0, 1, 3], np.float32), np.array([0, 8, 12], np.float32), np.array([2, 13, 20], np.float32)
    for stats in (FR.emulate, FR.exact):
        r = FR.report(T, S, H, probs=(0.0, 0.25, 0.5, 1.0), stats=stats)
        assert r["aa_truth"] == 1 / 3 and r["aa_synth"] == 2 / 3 and r["aa"] == 0.5 and r["n_exact_copies"] == 1
        assert r["aa_holdout"] == 1 / 3 and r["privacy_loss"] == pytest.approx(-1 / 6, rel=1e-15) and r["closer_to_train"] == 0.5
        assert r["dcr_quantiles"] == (0.0, 2.5, 5.0, 9.0)
        # S x T: 0+1+3, 8+7+5, 12+11+9 = 56;  S x S: 2 (8 + 12 + 4) = 48;  T x T: 2 (1 + 3 + 2) = 12
        assert r["energy_train"][0] == pytest.approx(2 * 56 / 9 - 48 / 9 - 12 / 9, rel=1e-14)
        assert r["energy_train"][1] == pytest.approx(2 * 56 / 9 - 48 / 6 - 12 / 6, rel=1e-14)
    assert "energy_holdout" not in FR.report(T, S) and "closer_to_train" not in FR.report(T, S)
