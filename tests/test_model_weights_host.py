"""d3p_amd.model_weights without a GPU: the module surface and its lazy import, the declared symbols, every refusal of the C entries and
of the Python layer before the device is touched, the workspace-size functions, and the numpy restatement (tests/model_weights_ref.py)
against cases solvable by hand and against the oracle's threefry."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import model_weights_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("model_weights reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


# ------------------------------------------------------------------------------------------------ surface
def test_module_surface_and_declared_symbols():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import criteria as CR
    from d3p_amd import model_weights as MW
    assert d3p_amd.model_weights is MW and "model_weights" in d3p_amd.__all__
    for name in ("stacking_weights", "pseudo_bma_weights", "compare_models", "stacking_from_matrix", "bootstrap_from_matrix"):
        assert name in MW.__all__ and callable(getattr(MW, name))
    assert MW.ModelWeights._fields == ("names", "weights", "method", "n_iter", "converged", "gap", "stacked_elpd", "se_boot")
    assert MW.ModelComparison._fields[:9] == ("names", "rank", "elpd", "p", "elpd_diff", "dse", "weight", "se", "warning")
    assert MW.METHODS == ("stacking", "pseudo-BMA", "pseudo-BMA+") and MW.MAX_MODELS == 16 and MW.MAX_BOOT == 65535
    assert CR.__all__ == ["waic", "posterior_waic", "compare", "WAICResult", "ComparisonResult"]          # (untouched)
    assert CR.ComparisonResult._fields == ("elpd_diff", "se_diff")
    hdr = open(os.path.join(ROOT, "include", "d3p_hip.h")).read()
    arity = {"d3p_stacking_workspace": 2, "d3p_stacking_weights": 11, "d3p_stacking_set_chunk": 1, "d3p_stacking_strip_rows": 0,
             "d3p_bb_pseudo_bma_workspace": 3, "d3p_bb_pseudo_bma": 11, "d3p_bb_pseudo_bma_strip_rows": 0}
    for name, n in arity.items():
        m = re.search(r"\b(?:int|size_t|uint32_t) " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        args = m.group(1).strip()
        assert (0 if args == "void" else args.count(",") + 1) == n == len(L.SIGNATURES[name][1]), name
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    assert any(p.endswith("d3p_model_weights.hip") for p in L._SRC) and all(p in L._DEPS for p in L._SRC)
    lib = L.load()
    assert lib.d3p_abi_version() == 9 and all(hasattr(lib, name) for name in arity)
    assert lib.d3p_stacking_strip_rows() == 256 and lib.d3p_bb_pseudo_bma_strip_rows() == 256
    text = open(os.path.join(ROOT, "d3p_amd", "csrc", "d3p_model_weights.hip")).read()
    assert "d3p_colreduce.h" not in text and "hipFuncSetAttribute" not in text and "oracle" not in text and "atomic" not in text.replace(
        "No atomics", "")
    assert re.findall(r'#include "([^"]+)"', text) == ["d3p_device.h", "d3p_host.h"]
    assert "FLOAT64 log" in text                                                   # the source says which logarithm
    for doc, pat in (("INTEGRATION.md", r"`d3p_stacking_weights`[^\n]*loo_model_weights"), ("README.md", r"model_weights"),
                     ("DESIGN.md", r"4r\.")):
        assert re.search(pat, open(os.path.join(ROOT, doc)).read()), doc


def test_import_stays_lazy():
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.model_weights' not in sys.modules; " \
           "d3p_amd.model_weights; assert 'd3p_amd.model_weights' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------------------------------------ the C entries' refusals
def test_the_c_entries_refuse_on_the_host_as_declared():
    """Everything both entries check before they ask whether a pointer is device memory, and that question itself: the buffers here are
    host memory and are never reached."""
    import d3p_amd._lib as L
    lib = L.load()
    buf = np.zeros(4096, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    odd4, odd2 = C.c_void_p(buf.ctypes.data + 4), C.c_void_p(buf.ctypes.data + 2)
    big = 1 << 20

    def stack(e=p, ld=8, rows=8, M=3, tol=1e-6, max_iter=10, w=p, info=p, ws=p, nbytes=big):
        return lib.d3p_stacking_weights(None, e, ld, rows, M, tol, max_iter, w, info, ws, nbytes)

    def boot(key=p, e=p, ld=8, rows=8, M=3, B=10, w=p, z=p, ws=p, nbytes=big):
        return lib.d3p_bb_pseudo_bma(None, key, e, ld, rows, M, B, w, z, ws, nbytes)
    for run, names in ((stack, ("e", "w", "info", "ws")), (boot, ("key", "e", "w", "z", "ws"))):
        for name in names:
            assert run(**{name: None}) == -1 and b"null" in lib.d3p_last_error(), name
            assert run(**{name: odd2}) == -1 and b"aligned" in lib.d3p_last_error(), name
        for name in names[-3:]:                                                   # the float64 arrays: 8 bytes
            assert run(**{name: odd4}) == -1 and b"aligned to 8" in lib.d3p_last_error(), name
        assert run(e=odd4) in (-1,) and b"device memory" in lib.d3p_last_error()   # 4-byte alignment is enough for e
        for M in (0, 17, 2 ** 32 - 1):
            assert run(M=M) == -1 and b"1 <= M <= 16" in lib.d3p_last_error()
        assert run(rows=0, ld=0) == -1 and b"rows >= 1" in lib.d3p_last_error()
        assert run(ld=7) == -1 and run(ld=-1) == -1 and b"ld >= rows" in lib.d3p_last_error()
        assert run(rows=2 ** 32, ld=2 ** 32) == -3 and b"2^32 - 1" in lib.d3p_last_error()
        assert run() == -1 and b"device memory" in lib.d3p_last_error()           # every value is fine; the memory is the host's
    for tol in (0.0, -1e-6, float("nan")):
        assert stack(tol=tol) == -1 and b"tol > 0" in lib.d3p_last_error()
    assert stack(max_iter=0) == -1 and b"max_iter >= 1" in lib.d3p_last_error()
    for B in (0, 65536, 2 ** 32 - 1):
        assert boot(B=B) == -1 and b"1 <= B <= 65535" in lib.d3p_last_error()
    need = lib.d3p_stacking_workspace(8, 3)
    assert stack(nbytes=need - 1) == -4 and b"workspace too small" in lib.d3p_last_error()
    need = lib.d3p_bb_pseudo_bma_workspace(8, 3, 10)
    assert boot(nbytes=need - 1) == -4 and b"workspace too small" in lib.d3p_last_error()
    assert not buf.any()
    before = lib.d3p_stacking_set_chunk(0)
    assert before >= 64 and lib.d3p_stacking_set_chunk(64) == 128 and lib.d3p_stacking_set_chunk(0) == 64
    for n in (1, 63, -5):
        assert lib.d3p_stacking_set_chunk(n) == -1 and b"at least 64" in lib.d3p_last_error()
    assert lib.d3p_stacking_set_chunk(before) == 128


def test_workspace_sizes_are_monotone():
    import d3p_amd._lib as L
    lib = L.load()
    rows = (1, 255, 256, 257, 513, 10 ** 4, 131072, 131073, 10 ** 6, 10 ** 7, 2 ** 32 - 1)
    for M in (1, 2, 16):
        sizes = [lib.d3p_stacking_workspace(r, M) for r in rows]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] >= 17 * 8 + (M + 1) * 8
        assert max(sizes) <= 17 * 8 + 512 * (M + 1) * 8 + 8                        # at most 512 strips: no rows x M array
        for B in (1, 1000):
            sizes = [lib.d3p_bb_pseudo_bma_workspace(r, M, B) for r in rows]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] == (M + 1 + M) * B * 8
            assert max(sizes) <= (128 * (M + 1) + M) * B * 8                        # at most 128 strips: no B x rows array
    for r in rows:
        assert all(lib.d3p_stacking_workspace(r, M) < lib.d3p_stacking_workspace(r, M + 1) for M in range(1, 16))
        assert all(lib.d3p_bb_pseudo_bma_workspace(r, M, 7) < lib.d3p_bb_pseudo_bma_workspace(r, M + 1, 7) for M in range(1, 16))
        assert all(lib.d3p_bb_pseudo_bma_workspace(r, 3, B) < lib.d3p_bb_pseudo_bma_workspace(r, 3, B + 1) for B in (1, 255, 256, 65534))


# ------------------------------------------------------------------------------------------------ the Python layer's refusals
def _loo(rows=6, pointwise=True, high=0):
    from d3p_amd.criteria import LOOResult
    z = torch.zeros((), dtype=torch.float64)
    pw = {k: torch.zeros(rows) for k in ("elpd_loo", "p_loo", "lppd", "pareto_k")} if pointwise else None
    return LOOResult(z, z, z, z, 4, rows, 0.7, torch.tensor(high), pw)


def _waic(rows=6, pointwise=True):
    from d3p_amd.criteria import WAICResult
    z = torch.zeros((), dtype=torch.float64)
    pw = {k: torch.zeros(rows) for k in ("lppd", "p_waic", "elpd_waic")} if pointwise else None
    return WAICResult(z, z, z, z, 4, rows, pw)


def test_python_layer_refuses_before_the_device(no_device):
    from d3p_amd import model_weights as MW
    good = {"a": _loo(), "b": _loo()}
    key = torch.zeros(2, dtype=torch.int32)                                        # (a CPU tensor: not a key of this package)
    for fn in (MW.stacking_weights, MW.pseudo_bma_weights, MW.compare_models):
        with pytest.raises(ValueError, match="different quantities"):
            fn({"a": _loo(), "b": _waic()})
        with pytest.raises(ValueError, match="pointwise=True"):
            fn({"a": _loo(), "b": _loo(pointwise=False)})
        with pytest.raises(ValueError, match="pointwise=True"):
            fn([_waic(), 3.0])
        with pytest.raises(ValueError, match="the same rows"):
            fn([_waic(6), _waic(7)])
        with pytest.raises(ValueError, match="1 <= M <= 16"):
            fn([_loo()] * 17)
        with pytest.raises(ValueError, match="1 <= M <= 16"):
            fn({})
        with pytest.raises(ValueError, match="dict or a list"):
            fn(_loo())
    for kw in ({"tol": 0.0}, {"tol": -1.0}, {"tol": float("nan")}, {"tol": "x"}, {"max_iter": 0}, {"max_iter": 2.5}, {"max_iter": True}):
        with pytest.raises(ValueError, match="tol|max_iter"):
            MW.stacking_weights(good, **kw)
        with pytest.raises(ValueError, match="tol|max_iter"):
            MW.compare_models(good, **kw)
    for n_boot in (0, 65536, 2.0, True):
        with pytest.raises(ValueError, match="n_boot"):
            MW.pseudo_bma_weights(good, rng_key=key, n_boot=n_boot)
    with pytest.raises(TypeError, match="threefry"):
        MW.pseudo_bma_weights(good, rng_key=key)
    with pytest.raises(ValueError, match="method"):
        MW.compare_models(good, method="bma")
    with pytest.raises(ValueError, match="rng_key"):
        MW.compare_models(good, method="pseudo-BMA+")
    with pytest.raises(ValueError, match="no further arguments"):
        MW.compare_models(good, method="pseudo-BMA", n_boot=3)
    e = torch.zeros((3, 8))
    for bad in (e[0], e.double(), torch.zeros((17, 8)), torch.zeros((3, 0)), e, np.zeros((3, 8), np.float32)):
        with pytest.raises(ValueError, match="e must|1 <= M|rows >= 1"):
            MW.stacking_from_matrix(bad)
        with pytest.raises(ValueError, match="e must|1 <= M|rows >= 1"):
            MW.bootstrap_from_matrix(key, bad)
    with pytest.raises(ValueError, match="tol"):
        MW.stacking_from_matrix(e, tol=0)
    with pytest.raises(ValueError, match="n_boot"):
        MW.bootstrap_from_matrix(key, e, n_boot=0)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_threefry_is_the_oracles():
    from oracle import oracle
    rng = np.random.default_rng(5)
    words = rng.integers(0, 2 ** 32, (40, 4), dtype=np.uint64).astype(np.uint32)
    words[0] = 0
    words[1] = 0xFFFFFFFF
    for k0, k1, c0, c1 in words:
        want = oracle.threefry2x32(int(k0), int(k1), int(c0), int(c1))
        got = R.threefry2x32(k0, k1, np.array([c0]), np.array([c1]))
        assert (int(got[0][0]), int(got[1][0])) == (int(want[0]), int(want[1]))
    # the stream's layout: word (r & 1) of the call at (r >> 1, b); replicate b does not depend on B, b0 or rows
    key = np.array([0x1234, 0xBEEF], np.uint32)
    bits = R.bb_bits(key, 3, 7)
    for b in range(3):
        for r in range(7):
            assert int(bits[b, r]) == int(oracle.threefry2x32(int(key[0]), int(key[1]), r >> 1, b)[r & 1])
    assert (R.bb_bits(key, 1, 5, b0=2) == bits[2:3, :5]).all()
    # the float32 uniform rule: [0, 1), multiples of 2^-23, and 1 - u exact
    u = R.bits_to_uniform(np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], np.uint32))
    assert u.dtype == np.float32 and u.tolist() == [0.0, 0.0, 2.0 ** -23, 1.0 - 2.0 ** -23]
    g = R.bb_weights(key, 4, 100)
    assert g.dtype == np.float64 and (g >= 0).all() and np.isfinite(g).all()


def test_restatement_on_cases_solvable_by_hand():
    rng = np.random.default_rng(0)
    one = rng.normal(-1.0, 1.0, (1, 50)).astype(np.float32)
    w, j, conv, gap, f = R.stacking(one, 1e-9, 100)
    assert w.tolist() == [1.0] and j == 0 and conv and gap == 0.0 and f == pytest.approx(one.astype(np.float64).sum(), rel=1e-15)
    # one model dominates every row: w -> (1, 0); the gap's certificate holds and f rises to the dominant model's total
    dom = np.stack([one[0], one[0] - np.float32(0.5) - rng.random(50).astype(np.float32)])
    w, j, conv, gap, f = R.stacking(dom, 1e-9, 20000)
    assert conv and 0 < j < 20000 and w[0] > 1 - 1e-8 and w[1] < 1e-8 and gap <= 1e-9
    assert -1e-10 <= dom[0].astype(np.float64).sum() - f <= 50 * gap + 1e-10
    # two identical models: the gap is 0 at the start and the weights stay at 1/2
    w, j, conv, gap, f = R.stacking(np.stack([one[0], one[0]]), 1e-12, 100)
    assert w.tolist() == [0.5, 0.5] and j == 0 and conv and gap == 0.0
    # the cut-off: n_iter = max_iter, not converged, and the gap is the returned w's
    w, j, conv, gap, f = R.stacking(dom, 1e-9, 5)
    assert j == 5 and not conv and gap == pytest.approx(R.stacking_gap(dom, w), abs=1e-14)
    # EM ascends monotonically and the gap bounds the distance to the optimum
    e = (rng.normal(-1.5, 1.0, 300)[None, :] + rng.normal(0, 0.5, (4, 300))).astype(np.float32)
    fs = [R.stacking(e, 1e-12, k)[4] for k in range(0, 30, 3)]
    assert all(a <= b + 1e-10 for a, b in zip(fs, fs[1:]))
    best = R.stacking(e, 1e-10, 50000)
    for k in (0, 3, 30):
        w, j, conv, gap, f = R.stacking(e, 1e-12, k)
        assert (best[4] - f) / 300 <= gap + 1e-12
    # special values
    bad = e.copy()
    bad[2, 17] = np.nan
    assert np.isnan(R.stacking(bad)[0]).all() and np.isnan(R.bb_pseudo_bma((1, 2), bad, 5)[0]).all()
    bad = e.copy()
    bad[:, 5] = -np.inf
    assert np.isnan(R.stacking(bad)[0]).all() and np.isnan(R.bb_pseudo_bma((1, 2), bad, 5)[1]).all()
    bad = e.copy()
    bad[1, 0] = np.inf
    assert np.isnan(R.stacking(bad)[0]).all() and np.isnan(R.bb_pseudo_bma((1, 2), bad, 5)[0]).all()
    some = e.copy()
    some[3, 4] = -np.inf
    w, j, conv, gap, f = R.stacking(some, 1e-6)
    assert conv and np.isfinite(w).all() and abs(w.sum() - 1) < 1e-12              # (stacking: the other models cover that row)
    wb, z, _ = R.bb_pseudo_bma((1, 2), some, 5)
    assert (z[:, 3] == -np.inf).all() and np.isfinite(z[:, :3]).all() and wb[3] == 0.0 and abs(wb.sum() - 1) < 1e-12


def test_restatement_bootstrap_is_a_bootstrap():
    rng = np.random.default_rng(1)
    e = (rng.normal(-1.5, 1.0, 200)[None, :] + rng.normal(0, 0.5, (3, 200))).astype(np.float32)
    w, z, scale = R.bb_pseudo_bma((7, 9), e, 400)
    assert z.shape == (400, 3) and abs(w.sum() - 1) < 1e-12 and (scale > 0).all()
    total = e.astype(np.float64).sum(axis=1)
    assert (np.abs(z.mean(axis=0) - total) < 5 * z.std(axis=0) / np.sqrt(400)).all()
    # the replicates' spread is the elpd's standard error (Rubin 1981): sqrt(rows Var_r e) up to the bootstrap's own noise
    se = np.sqrt(200 * e.astype(np.float64).var(axis=1))
    assert (np.abs(z.std(axis=0) / se - 1) < 0.25).all()
