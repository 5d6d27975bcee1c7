"""d3p_amd.energy without a GPU: the module surface and its lazy import, the declared symbols and query functions, every refusal of the C
entry and of the Python layer before the device is touched, the source-text rules of d3p_energy.hip, and the numpy emulation of the
kernel's rule (tests/energy_ref.py) against the derived bound -- including draws clustered far from the origin, the case a Gram-matrix
distance would lose -- and against cases solvable by hand."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import energy_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("energy reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


# ------------------------------------------------------------------------------------------------ surface
def test_module_surface_and_declared_symbols():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import energy as E
    from d3p_amd import mixture as MX
    from d3p_amd import scoring as SC
    assert d3p_amd.energy is E and d3p_amd.__all__[-1] == "energy"
    for name in ("energy_score_draws", "energy_score", "draws_limit", "posterior_predictive_energy_score", "compare_energy_scores"):
        assert name in E.__all__ and callable(getattr(E, name))
    assert E.EnergyScoreResult._fields == ("es", "se", "mae", "spread", "n_draws", "n_rows", "dim", "pointwise")
    assert E.EnergyScoreComparison._fields == ("es_diff", "se_diff") and E.INT_EXACT == 2 ** 24
    assert SC.__all__[:2] == ["score_draws", "crps"] and "energy_score" not in SC.__all__ and len(SC.__all__) == 10       # (untouched)
    assert MX.__all__[-1] == "ROW_TILE" and len(MX.__all__) == 6                                                           # (untouched)
    hdr = open(os.path.join(ROOT, "include", "d3p_hip.h")).read()
    arity = {"d3p_energy_score": 12, "d3p_energy_score_max_n": 0, "d3p_energy_score_tile_draws": 0, "d3p_energy_score_chunk_cols": 0,
             "d3p_energy_score_rows_per_group": 1, "d3p_energy_score_form": 3, "d3p_energy_score_set_form": 1}
    for name, n in arity.items():
        m = re.search(r"\b(?:int|uint32_t) " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).strip()
        assert (0 if args == "void" else args.count(",") + 1) == n == len(L.SIGNATURES[name][1]), name
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    assert any(p.endswith("d3p_energy.hip") for p in L._SRC) and all(p in L._DEPS for p in L._SRC)
    lib = L.load()
    assert lib.d3p_abi_version() == 9 and all(hasattr(lib, name) for name in arity)
    for doc, pat in (("INTEGRATION.md", r"`d3p_energy_score`"), ("README.md", r"d3p_amd\.energy|energy score"), ("DESIGN.md", r"4v\."),
                     (os.path.join("docs", "experiments_energy.md"), r"energy")):
        assert re.search(pat, open(os.path.join(ROOT, doc)).read()), doc


def test_import_stays_lazy():
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.energy' not in sys.modules; " \
           "d3p_amd.energy; assert 'd3p_amd.energy' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_query_functions_and_the_form_aid():
    import d3p_amd._lib as L
    from d3p_amd import energy as E
    lib = L.load()
    T, Cc = lib.d3p_energy_score_tile_draws(), lib.d3p_energy_score_chunk_cols()
    assert T >= 8 and Cc >= 4 and Cc % 4 == 0
    assert lib.d3p_energy_score_max_n() == E.draws_limit() == 65535
    R = lib.d3p_energy_score_rows_per_group(1)
    assert R > 1 and R * 2 * 4 >= 128                               # at the example's d = 2 a workgroup's rows cover a 128-byte line
    assert lib.d3p_energy_score_rows_per_group(2) == 1
    assert lib.d3p_energy_score_rows_per_group(0) == 0 and lib.d3p_energy_score_rows_per_group(3) == 0
    try:
        assert lib.d3p_energy_score_set_form(0) == 0
        for n, rows, d in ((1, 1, 1), (100, 2048, 2), (128, 8192, 64), (64, 512, 784), (65535, 1, 1), (100, 10 ** 6, 2)):
            assert lib.d3p_energy_score_form(n, rows, d) in (1, 2), (n, rows, d)
        assert lib.d3p_energy_score_form(64, 512, 784) == 2         # the VAE's d: one row per workgroup, streamed
        assert lib.d3p_energy_score_form(100, 10 ** 6, 2) == 1      # many short rows: several rows per workgroup
        assert lib.d3p_energy_score_form(0, 4, 2) == 0 and lib.d3p_energy_score_form(65536, 4, 2) == 0 and lib.d3p_energy_score_form(4, 4, 0) == 0
        for form in (1, 2):
            assert lib.d3p_energy_score_set_form(form) == 0
            assert lib.d3p_energy_score_form(100, 2048, 2) == form and lib.d3p_energy_score_form(64, 512, 784) == form
        for form in (-1, 3, 7):
            assert lib.d3p_energy_score_set_form(form) == -1 and b"form must be" in lib.d3p_last_error()
    finally:
        assert lib.d3p_energy_score_set_form(0) == 0


# ------------------------------------------------------------------------------------------------ the C entry's refusals
def test_the_c_entry_refuses_on_the_host_as_declared():
    """Everything the entry checks before it asks whether a pointer is device memory, and that question itself: the buffers here are
    host memory and are never reached."""
    import d3p_amd._lib as L
    lib = L.load()
    buf = np.zeros(4096, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    odd = C.c_void_p(buf.ctypes.data + 2)

    def run(z=p, dtype=0, ld_draw=24, ld_row=3, n=5, rows=8, d=3, y=p, y_ld=3, out=p, out_ld=8):
        return lib.d3p_energy_score(None, z, dtype, ld_draw, ld_row, n, rows, d, y, y_ld, out, out_ld)
    for name in ("z", "y", "out"):
        assert run(**{name: None}) == -1 and b"null pointer" in lib.d3p_last_error(), name
        assert run(**{name: odd}) == -1 and b"not aligned to 4 bytes" in lib.d3p_last_error(), name
    for dtype in (-1, 2):
        assert run(dtype=dtype) == -1 and b"dtype must be 0 (float32) or 1 (int32)" in lib.d3p_last_error()
    assert run(n=0) == -1 and b"n >= 1" in lib.d3p_last_error()
    assert run(d=0, ld_row=0) == -1 and b"d >= 1" in lib.d3p_last_error()
    for ld_row in (2, -1):
        assert run(ld_row=ld_row) == -1 and b"ld_row >= d" in lib.d3p_last_error()
    for ld_draw in (23, -1, 0):
        assert run(ld_draw=ld_draw) == -1 and b"ld_draw >= rows * ld_row" in lib.d3p_last_error()
    assert run(rows=2 ** 62, ld_draw=2 ** 62, out_ld=2 ** 62) == -1 and b"ld_draw >= rows * ld_row" in lib.d3p_last_error()   # (no wrap)
    for y_ld in (2, -1):
        assert run(y_ld=y_ld) == -1 and b"y_ld >= d" in lib.d3p_last_error()
    for out_ld in (7, -1):
        assert run(out_ld=out_ld) == -1 and b"out_ld >= rows" in lib.d3p_last_error()
    for n in (65536, 2 ** 32 - 1):
        assert run(n=n) == -3 and b"n <= 65535" in lib.d3p_last_error()
    big = 2 ** 33
    try:
        assert lib.d3p_energy_score_set_form(2) == 0
        assert run(rows=big, ld_draw=3 * big, out_ld=big) == -3 and b"2^31 - 1 workgroups" in lib.d3p_last_error()
    finally:
        assert lib.d3p_energy_score_set_form(0) == 0
    assert run(rows=0, ld_draw=0, out_ld=0) == 0                    # nothing to do: no launch, and the pointers are not even asked about
    for dtype in (0, 1):
        assert run(dtype=dtype) == -1 and b"must be device memory" in lib.d3p_last_error()   # every value is fine; the memory is the host's
    assert not buf.any()


# ------------------------------------------------------------------------------------------------ the Python layer's refusals
def test_python_layer_refuses_before_the_device(no_device):
    from d3p_amd import energy as E
    from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel, LogisticRegression
    z = torch.zeros((5, 8, 3))
    y = torch.zeros((8, 3))
    for fn in (E.energy_score_draws, E.energy_score):
        for bad in (np.zeros((5, 8, 3), np.float32), z[0, 0], z[None], z.double(), z.to(torch.int64), torch.zeros((0, 8, 3)),
                    torch.zeros((5, 8, 0))):
            with pytest.raises(ValueError, match="draws: a 3-D float32 or int32 CUDA tensor|at least one draw|d >= 1"):
                fn(bad, y)
        with pytest.raises(ValueError, match="at most 65535 draws"):
            fn(torch.zeros((65536, 1, 1)), torch.zeros((1, 1)))
        with pytest.raises(ValueError, match="unit stride"):
            fn(torch.zeros((5, 3, 8)).transpose(1, 2), y)
        with pytest.raises(ValueError, match="overlap or are not in"):
            fn(torch.zeros((8, 5, 3)).transpose(0, 1), torch.zeros((8, 3)))
        with pytest.raises(ValueError, match="overlap or are not in"):
            fn(torch.zeros((1, 8, 3)).expand(5, 8, 3), y)
        for bad_y in (torch.zeros((8,)), torch.zeros((3, 8)), torch.zeros((8, 3, 1)), np.zeros((7, 3))):
            with pytest.raises(ValueError, match=r"y: shape \(8, 3\) expected"):
                fn(z, bad_y)
        with pytest.raises(ValueError, match="y must hold"):
            fn(z, torch.zeros((8, 3), dtype=torch.bool))
        with pytest.raises(ValueError, match="non-integral"):
            fn(z.to(torch.int32), torch.full((8, 3), 0.5))
        with pytest.raises(ValueError, match="CUDA tensor"):          # every value is fine; the tensor is the host's
            fn(z, y)
        with pytest.raises(ValueError, match="CUDA tensor"):
            fn(torch.zeros((5, 8)), torch.zeros(8))                   # (the 2-D form, d = 1)
    model = GaussianMixtureModel()
    guide = GaussianMixtureGuide(model)
    params = {"alpha_log": torch.zeros(3), "mus_loc": torch.zeros((3, 2))}
    key = torch.zeros(2, dtype=torch.int32)                            # (a CPU tensor: not a key of this package)
    obs = torch.zeros((130, 2))
    run = E.posterior_predictive_energy_score
    lr = LogisticRegression(2)
    with pytest.raises(TypeError, match="unsupported model LogisticRegression"):
        run(key, 5, lr, (obs, None), guide, params)
    with pytest.raises(TypeError, match="guide must be a GaussianMixtureGuide"):
        run(key, 5, model, (3, obs), None, params)
    with pytest.raises(TypeError, match="guide must be a GaussianMixtureGuide"):
        run(key, 5, model, (3, obs), lr, params)
    for n in (0, -3):
        with pytest.raises(ValueError, match="n must be >= 1"):
            run(key, n, model, (3, obs), guide, params)
    with pytest.raises(ValueError, match="n must be an int >= 1"):
        run(key, None, model, (3, obs), guide, params)
    with pytest.raises(ValueError, match="at most 65535 draws"):
        run(key, 65536, model, (3, obs), guide, params)
    with pytest.raises(ValueError, match="obs\\) is required"):
        run(key, 5, model, (3, None, 130, 2), guide, params)
    with pytest.raises(ValueError, match="obs\\) is required"):
        run(key, 5, model, (3,), guide, params)
    with pytest.raises(ValueError, match="slab_bytes >= 5200, got 5199"):
        run(key, 5, model, (3, obs), guide, params, slab_bytes=5199)
    for slab in (0, 2.5, True):
        with pytest.raises(ValueError, match="slab_bytes must be an int"):
            run(key, 5, model, (3, obs), guide, params, slab_bytes=slab)
    with pytest.raises(ValueError, match="params"):
        run(key, 5, model, (3, obs), guide, {"alpha_log": torch.zeros(3)})
    with pytest.raises(TypeError, match="threefry"):                   # the last host check: everything else was fine
        run(key, 5, model, (3, obs), guide, params)
    z64 = torch.zeros((), dtype=torch.float64)
    full = E.EnergyScoreResult(z64, z64, z64, z64, 5, 6, 2, {k: torch.zeros(6) for k in ("es", "mae", "spread")})
    for a, b in ((full, full._replace(pointwise=None)), (full._replace(pointwise=None), full), (full, 3.0)):
        with pytest.raises(ValueError, match="pointwise=True"):
            E.compare_energy_scores(a, b)
    with pytest.raises(ValueError, match="the same rows"):
        E.compare_energy_scores(full, full._replace(n_rows=7))
    with pytest.raises(ValueError, match="the same rows"):
        E.compare_energy_scores(full, full._replace(dim=3))
    a = full._replace(pointwise={"es": torch.tensor([1.0, 2.0, 4.0])}, n_rows=3)
    b = full._replace(pointwise={"es": torch.tensor([2.0, 2.0, 2.0])}, n_rows=3)
    cmp = E.compare_energy_scores(a, b)
    assert cmp.es_diff.dtype == torch.float64 and float(cmp.es_diff) == pytest.approx(1.0 / 3.0, rel=1e-15)
    assert float(cmp.se_diff) == pytest.approx(np.std([-1.0, 0.0, 2.0], ddof=1) / np.sqrt(3.0), rel=1e-14)
    assert float(E.compare_energy_scores(b, a).es_diff) == -float(cmp.es_diff)      # negative favours the first


# ------------------------------------------------------------------------------------------------ the source's own rules
def test_source_text_rules():
    csrc = os.path.join(ROOT, "d3p_amd", "csrc")
    text = open(os.path.join(csrc, "d3p_energy.hip")).read()
    tile = open(os.path.join(csrc, "d3p_pair_tile.h")).read()          # the 32 x 32 pair tile, shared with d3p_pair_stats.hip
    assert re.findall(r'#include "([^"]+)"', text) == ["d3p_device.h", "d3p_host.h", "d3p_pair_tile.h"]
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    tile_code = "\n".join(line.split("//")[0] for line in tile.splitlines())
    for banned in ("hipFuncSetAttribute", "147456", "atomic", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy",
                   "mfma", "extern __shared__", "workspace"):
        assert banned not in code and banned not in tile_code, banned
    header = text[:text.index("#include")]
    for said in ("THE RULE", "THE ORDER", "DETERMINISM", "fmaf chain", "2^24", "follow IEEE", "NaN or +-inf", "bit for bit", "Gram matrix"):
        assert said in header, said
    # the chain is the tile's (tests/test_fidelity_host.py pins its text there); the root is this file's own
    assert tile_code.count("__fmaf_rn(") == 4 and "__fmaf_rn(" not in code and "pair_chain(" in code
    assert "__fsqrt_rn(" in code and "sqrtf(" not in code.replace("__fsqrt_rn(", "") and "sqrt" not in tile_code
    assert not re.search(r"#define D3P_(ES|PS)_(T|C|LD|WAVES)\b", text)
    num = {k: int(re.search(r"#define D3P_PAIR_" + k + r" (\d+)", tile).group(1)) for k in ("T", "C", "LD", "WAVES")}
    lds = num["T"] * num["LD"] * 4 * 2 * num["WAVES"]
    assert lds + 1024 <= 64 * 1024                                    # static LDS stays below 64 KiB
    assert lds + num["WAVES"] * (2 * 8 + 4) == 36944 and "Static LDS: 36944 bytes at most" in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("4v."):]
    for said in ("Gram", "variogram", "rank histogram", "PSIS", "VGPR", "bit for bit"):
        assert said in section, said


# ------------------------------------------------------------------------------------------------ the restatement
def _cases():
    rng = np.random.default_rng(11)
    yield "normal", rng.normal(size=(33, 5, 3)).astype(np.float32), rng.normal(size=(5, 3)).astype(np.float32)
    far = (1.0e4 + 1.0e-3 * rng.normal(size=(40, 4, 2))).astype(np.float32)
    yield "clustered far from the origin", far, (1.0e4 + 1.0e-3 * rng.normal(size=(4, 2))).astype(np.float32)
    yield "0/1 at d = 784", rng.integers(0, 2, (6, 2, 784)).astype(np.int32), rng.integers(0, 2, (2, 784)).astype(np.int32)
    scale = (10.0 ** np.linspace(-6, 6, 13)).astype(np.float32)
    yield "columns over 12 decades", (rng.normal(size=(20, 3, 13)) * scale).astype(np.float32), (rng.normal(size=(3, 13)) * scale).astype(np.float32)
    yield "one draw", rng.normal(size=(1, 4, 2)).astype(np.float32), rng.normal(size=(4, 2)).astype(np.float32)
    yield "d = 1", rng.normal(size=(17, 6)).astype(np.float32), rng.normal(size=(6,)).astype(np.float32)


@pytest.mark.parametrize("name,draws,y", list(_cases()), ids=[c[0] for c in _cases()])
def test_emulation_lies_within_the_derived_bound(name, draws, y):
    n = draws.shape[0]
    d = draws.shape[2] if draws.ndim == 3 else 1
    ex, em = ER.exact(draws, y), ER.emulate(draws, y)
    tol = ER.bound(ex, n, d)
    worst = 0.0
    for k in ER.NAMES:
        if n == 1 and k == "es_fair":
            assert np.isnan(ex[k]).all() and np.isnan(em[k]).all()
            continue
        err = np.abs(em[k].astype(np.float64) - ex[k])
        assert (err <= tol[k]).all(), (name, k, float((err / tol[k]).max()))
        worst = max(worst, float((err / tol[k]).max()))
    print(f"{name}: largest error / bound {worst:.3f}")
    if name == "clustered far from the origin":
        # what the bound is for: a Gram-matrix distance |a|^2 + |b|^2 - 2 a.b in float32 loses these distances entirely
        z = draws[:, 0, :].astype(np.float32)
        sq = (z * z).sum(axis=1, dtype=np.float32)
        gram = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - np.float32(2) * (z @ z.T), 0)).astype(np.float64)
        iu = np.triu_indices(n, 1)
        spread_gram = 2.0 * gram[iu].sum() / (2.0 * n * n)
        assert abs(spread_gram - ex["spread"][0]) > 100 * tol["spread"][0]


def test_restatement_on_cases_solvable_by_hand():
    # d = 1 with small integers: draws 0, 1, 3 against y = 2: S1 = 2 + 1 + 1, S2 = 2 (1 + 3 + 2)
    z = np.array([0, 1, 3], np.int32)[:, None]
    for f in (ER.exact, ER.emulate):
        out = f(z, np.array([2], np.int32))
        assert out["mae"][0] == np.float32(4 / 3) or out["mae"][0] == 4 / 3
        assert float(out["spread"][0]) == pytest.approx(12 / 18, rel=1e-7) and float(out["es_fair"][0]) == pytest.approx(4 / 3 - 1.0, rel=1e-6)
    # d = 2, points k (3, 4): every distance is 5 |k_i - k_j|
    k = np.array([0, 2, -1, 5], np.float32)
    z = (k[:, None] * np.array([3, 4], np.float32))[:, None, :]
    out = ER.emulate(z, np.array([[3, 4]], np.float32))
    k64 = k.astype(np.float64)
    S1 = 5 * np.abs(k64 - 1).sum()
    S2 = 5 * np.abs(k64[:, None] - k64[None, :]).sum()
    assert out["mae"][0] == np.float32(S1 / 4) and out["spread"][0] == np.float32(S2 / 32)
    assert out["es"][0] == np.float32(S1 / 4 - S2 / 32) and out["es_fair"][0] == np.float32(S1 / 4 - S2 / 24)
    # all draws equal to y: zeros, and es_fair = 0 - 0 / (2 n (n - 1)) = 0
    z = np.broadcast_to(np.array([1.5, -2.0], np.float32), (4, 1, 2))
    out = ER.emulate(z, np.array([[1.5, -2.0]], np.float32))
    assert all(out[name][0] == 0.0 for name in ER.NAMES)
    # special values: NaN by row; overflow of q follows IEEE
    z = np.zeros((3, 3, 2), np.float32)
    z[1, 0, 1] = np.nan
    z[:, 2, 0] = (1e30, -1e30, 0.0)
    yy = np.zeros((3, 2), np.float32)
    yy[1, 0] = np.inf
    out = ER.emulate(z, yy)
    assert all(np.isnan(out[name][:2]).all() for name in ER.NAMES)
    assert out["mae"][2] == np.inf and out["spread"][2] == np.inf and np.isnan(out["es"][2]) and np.isnan(out["es_fair"][2])
    assert np.isfinite(ER.exact(z, yy)["es"][2])
    out = ER.emulate(z[:1], yy)
    assert np.isnan(out["es_fair"][2]) and out["spread"][2] == 0.0 and out["es"][2] == out["mae"][2]      # n = 1
