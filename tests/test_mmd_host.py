"""d3p_amd.mmd without a GPU: surface, declaration and signatures, refusals in their stated order, the closing arithmetic of mmd."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import d3p_amd._lib as L
from tests import mmd_ref as MR

ARITY = {"d3p_kernel_sums": 17, "d3p_kernel_sums_workspace": 3, "d3p_kernel_sums_strip_rows": 0, "d3p_kernel_sums_group_tiles": 0,
         "d3p_kernel_sums_resident_cols": 0, "d3p_kernel_sums_max_bandwidths": 0, "d3p_kernel_sums_segments": 2,
         "d3p_kernel_sums_segment_tiles": 2, "d3p_kernel_sums_roundings": 2, "d3p_kernel_sums_set_segments": 1}


def test_surface_declaration_and_geometry():
    import d3p_amd
    from d3p_amd import mmd as M
    assert d3p_amd.mmd is M and "mmd" in d3p_amd.__all__ and M.__all__[:3] == ["kernel_sums", "mmd", "MMD"]
    assert M.MMD._fields[:6] == ("mmd2", "mmd2_unbiased", "kxy", "kxx", "kyy", "sigma2") and "witness_y" in M.MMD._fields
    assert "PRIVACY" in M.__doc__ and "NOT covered by the accountant" in M.__doc__ and "not covered" in M.mmd.__doc__
    with open(os.path.join(os.path.dirname(os.path.dirname(L.__file__)), "include", "d3p_hip.h")) as f:
        hdr = f.read()
    lib = L.load()
    assert lib.d3p_abi_version() == 9
    for name, n in ARITY.items():
        args = re.search(r"^(?:int|size_t|uint32_t) " + name + r"\(([^)]*)\)", hdr, re.M).group(1).strip()
        assert (0 if args == "void" else args.count(",") + 1) == n == len(L.SIGNATURES[name][1]) and hasattr(lib, name), name
    assert any(p.endswith("d3p_mmd.hip") for p in L._SRC) and all(p in L._DEPS for p in L._SRC)
    assert (lib.d3p_kernel_sums_strip_rows(), lib.d3p_kernel_sums_group_tiles(), lib.d3p_kernel_sums_resident_cols(), M.MAX_BANDWIDTHS) == (
        128, 64, 64, lib.d3p_kernel_sums_max_bandwidths())


def test_the_c_entry_refuses_on_the_host_in_the_stated_order():
    lib = L.load()
    buf = np.zeros(8192, np.float32)
    p, odd, odd4 = (C.c_void_p(buf.ctypes.data + k) for k in (0, 2, 4))
    need = lib.d3p_kernel_sums_workspace(40, 50, 2)

    def refused(rc, text, a=p, b=p, dtype=0, a_ld=3, b_ld=3, na=40, nb=50, d=3, shift=p, scale=p, gamma0=0.5, n_b=2, excl=0, out=p, ws=p,
                ws_bytes=1 << 20):
        assert lib.d3p_kernel_sums(None, a, b, dtype, a_ld, b_ld, na, nb, d, shift, scale, gamma0, n_b, excl, out, ws, ws_bytes) == rc
        assert text in lib.d3p_last_error(), text
    for name in ("a", "b", "out", "ws"):
        refused(-1, b"null pointer", **{name: None}, shift=odd)
    for name in ("a", "b", "shift", "scale"):
        refused(-1, b"not aligned to 4 bytes", **{name: odd}, out=odd4)
    for name in ("out", "ws"):
        refused(-1, b"not aligned to 8 bytes", **{name: odd4}, dtype=7)
    refused(-1, b"dtype must be 0 (float32) or 1 (int32)", dtype=2, na=0)
    refused(-1, b"na >= 1 and nb >= 1", nb=0, d=0)
    refused(-1, b"d >= 1", d=0, a_ld=-1)
    refused(-1, b"a_ld >= d", a_ld=2, b_ld=2)
    refused(-1, b"b_ld >= d", b_ld=2, excl=2)
    refused(-1, b"does not fit 63 bits", a_ld=2 ** 62, excl=2)
    refused(-1, b"exclude_diagonal must be 0 or 1", excl=2, n_b=0)
    refused(-1, b"na == nb is required", excl=1, n_b=0)
    refused(-1, b"n_bandwidths must be in 1 .. 8", n_b=9, gamma0=0.0)
    for g in (0.0, -1.0, float("inf"), float("nan")):
        refused(-1, b"gamma0 must be finite and > 0", gamma0=g, na=2 ** 31)
    refused(-3, b"at most 2^31 - 1 each", na=2 ** 31, ws_bytes=0)
    refused(-4, b"workspace too small", ws_bytes=need - 1)
    refused(-1, b"must be device memory", ws_bytes=need, shift=None, scale=None)       # every value is fine
    assert not buf.any() and lib.d3p_kernel_sums_set_segments(-1) == -1 and b"segments must be 0" in lib.d3p_last_error()
    for bad in ((0, 4, 1), (4, 0, 1), (2 ** 31, 4, 1), (4, 4, 0), (4, 4, 9)):
        assert lib.d3p_kernel_sums_workspace(*bad) == 0
    assert need == lib.d3p_kernel_sums_segments(40, 50) * 40 * (8 * 2 + 4) + 4 * 90


def test_python_layer_refuses_before_the_device(monkeypatch):
    from d3p_amd import mmd as M
    monkeypatch.setattr(L, "require_device", lambda: pytest.fail("mmd reached require_device"))
    z, zi = torch.zeros((40, 3)), torch.zeros((40, 3), dtype=torch.int32)
    cases = [("d >= 1", M.kernel_sums, (torch.zeros((8, 0)), z, 1.0), {}), ("unit stride", M.mmd, (z, torch.zeros((3, 40)).t()), {}),
             ("one dtype for both", M.kernel_sums, (z, zi, 1.0), {}), ("one d for both", M.mmd, (z, torch.zeros((5, 2))), {}),
             ("gamma0 must be a finite number > 0", M.kernel_sums, (z, z, 0.0), {}), ("gamma0 must be", M.kernel_sums, (z, z, float("nan")), {}),
             ("n_bandwidths must be an int in 1 .. 8", M.kernel_sums, (z, z, 1.0, 9), {}), ("n_bandwidths must be", M.mmd, (z, z), {"n_bandwidths": 0}),
             ("shift must be None or a contiguous float32", M.kernel_sums, (z, z, 1.0), {"shift": torch.zeros(6)[::2]}),
             ("scale must be None or a contiguous float32", M.kernel_sums, (z, z, 1.0), {"scale": torch.zeros(3, dtype=torch.float64)}),
             ("exclude_diagonal must be a bool", M.kernel_sums, (z, z, 1.0), {"exclude_diagonal": 2}),
             ("compares a table with itself", M.kernel_sums, (z, z[:5], 1.0), {"exclude_diagonal": True}),
             ("bandwidth must be 'median' or", M.mmd, (z, z), {"bandwidth": "scott"}), ("bandwidth must be a finite", M.mmd, (z, z), {"bandwidth": -1.0}),
             ("scale must be 'std' or None", M.mmd, (z, z), {"scale": "iqr"}), ("CUDA tensor", M.kernel_sums, (z, z, 1.0), {}),
             ("CUDA tensor", M.mmd, (z, z), {})]
    for match, fn, args, kw in cases:
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)


@pytest.mark.parametrize("n_y", [2, 1])
def test_closing_arithmetic_on_reference_row_sums(n_y):
    """x = {0, 1, 3}, y = {1/2, 2} (or {1/2}) on the line: the per-row sums come from the reference, the statistics from the definitions."""
    from d3p_amd import mmd as M
    x, y = np.array([[0.0], [1.0], [3.0]], np.float32), np.array([[0.5], [2.0]], np.float32)[:n_y]
    sigma2, gamma0 = M._ladder(0.8, 2)
    wide = M._ladder(3.0, 5)[0]                                    # the ladder: factor 2 a rung, the geometric centre the given sigma^2
    assert all(abs(wide[b] / wide[b + 1] - 2.0) < 1e-15 for b in range(4)) and abs(wide[0] * wide[4] - 9.0) < 1e-14 and abs(wide[2] - 3.0) < 1e-15
    sums = [torch.tensor(MR.kernel_sums(a, b, gamma0, 2, exclude=e)[0]) for a, b, e in ((x, y, False), (y, x, False), (x, x, True), (y, y, True))]
    got = M._closing(*sums, sigma2, 1)
    assert (got.n_x, got.n_y, got.dim) == (3, n_y, 1) and got.sigma2.tolist() == sigma2
    for b in range(2):
        s2 = 1.0 / (2.0 * np.log(2.0) * float(np.float32(gamma0)) * 2 ** b)               # (gamma0 as the kernel takes it: a float32)
        v, u, wx, wy = MR.mmd(x.astype(np.float64), y.astype(np.float64), s2)
        assert abs(float(got.mmd2[b]) - v) < 1e-14 and np.abs(got.witness_x[b].numpy() - wx).max() < 1e-14
        assert np.abs(got.witness_y[b].numpy() - wy).max() < 1e-14
        assert np.isnan(float(got.mmd2_unbiased[b])) if n_y == 1 else abs(float(got.mmd2_unbiased[b]) - u) < 1e-14
        # by hand: the V-statistic's diagonal is the exact n; x's own neighbourhood has more of x than of y (positive witness at 3)
        assert abs(float(got.kxx[b]) - (3.0 + 2.0 * sum(np.exp(-q / (2.0 * s2)) for q in (1.0, 9.0, 4.0))) / 9.0) < 1e-14
        assert n_y == 2 or float(got.witness_x[b][2]) > 0.0 > float(got.witness_y[b][0])
