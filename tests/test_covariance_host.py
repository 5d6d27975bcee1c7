"""d3p_amd.covariance without a GPU: the surface, the geometry of the query functions, every refusal of the C entry and the Python layer."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import d3p_amd._lib as L
from tests import covariance_ref as CR

ARITY = {"d3p_column_moments": 11, "d3p_column_moments_workspace": 2, "d3p_column_moments_block_cols": 0, "d3p_column_moments_strip_rows": 0,
         "d3p_column_moments_segment_rows": 2}


def test_module_surface_and_lazy_import():
    import d3p_amd
    from d3p_amd import covariance as CV
    names = d3p_amd.__all__
    assert d3p_amd.covariance is CV and names.index("covariance") < names.index("permutation") and names[-3:] == ["marginals", "fidelity", "energy"]
    assert CV.__all__ == ["column_moments", "covariance", "correlation", "correlation_fidelity", "ColumnMoments", "CorrelationFidelity", "INT_EXACT"]
    assert CV.ColumnMoments._fields == ("n", "mean", "m2") and CV.INT_EXACT == 2 ** 24 and set(CV.CorrelationFidelity._fields) >= {
        "smd", "sd_ratio", "worst_columns", "corr_diff_mean", "corr_diff_max", "corr_diff_frobenius", "worst_pairs", "n_pairs_skipped", "frechet", "floor"}
    assert "PRIVACY" in CV.__doc__ and "NOT covered by the accountant" in CV.__doc__ and "not covered" in CV.correlation_fidelity.__doc__
    lib = L.load()
    assert lib.d3p_abi_version() == 9 and all(len(L.SIGNATURES[name][1]) == n and hasattr(lib, name) for name, n in ARITY.items())
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.covariance' not in sys.modules; " \
           "d3p_amd.covariance; assert 'd3p_amd.covariance' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.mark.parametrize("n,d", [(1, 1), (2049, 129), (9, 784), (10 ** 5, 2), (10 ** 6, 64), (6 * 10 ** 4, 784), (2 ** 32 - 2, 1), (2 ** 32 - 2, 2000)])
def test_query_functions_give_the_geometry(n, d):
    lib = L.load()
    B, Ls, R, nseg = CR.geometry(lib, n, d)
    nb, pairs = -(-d // B), -(-d // B) * (-(-d // B) + 1) // 2
    assert B % 32 == 0 and R % (4 * Ls) == 0 and R >= 4 * Ls and nseg <= 1024 // min(pairs, 1024) + 1
    sum_seg = -(-n // lib.d3p_column_moments_segment_rows(n, 1))                # (the column sums' own segments: those of one block pair)
    assert lib.d3p_column_moments_workspace(n, d) == 8 * nb * B + 8 * sum_seg * nb * B + 8 * 2 * B * pairs + 8 * (B * B + 2 * B) * pairs * nseg
    for bad in ((0, 4), (4, 0), (2 ** 32 - 1, 4)):
        assert lib.d3p_column_moments_workspace(*bad) == 0 and lib.d3p_column_moments_segment_rows(*bad) == 0


def test_the_c_entry_refuses_on_the_host_as_declared():
    lib = L.load()
    buf = np.zeros(8192, np.float32)
    p, odd, odd4 = (C.c_void_p(buf.ctypes.data + k) for k in (0, 2, 4))
    need = lib.d3p_column_moments_workspace(40, 3)

    def refused(rc, text, x=p, dtype=0, ld=3, n=40, d=3, mean=p, m2=p, m2_ld=3, ws=p, ws_bytes=1 << 20):
        assert lib.d3p_column_moments(None, x, dtype, ld, n, d, mean, m2, m2_ld, ws, ws_bytes) == rc and text in lib.d3p_last_error(), text
    for name in ("x", "mean", "m2", "ws"):
        refused(-1, b"null pointer", **{name: None})
    refused(-1, b"not aligned to 4 bytes", x=odd)
    for name in ("mean", "m2", "ws"):
        refused(-1, b"not aligned to 8 bytes", **{name: odd4})
    refused(-1, b"null pointer", x=None, mean=odd4)             # the order: null, alignment, dtype, n, d, ld, m2_ld, grid, workspace
    refused(-1, b"not aligned", x=odd, dtype=7)
    for dtype in (-1, 2):
        refused(-1, b"dtype must be 0 (float32) or 1 (int32)", dtype=dtype, n=0)
    for n in (0, 2 ** 32 - 1, 2 ** 40):
        refused(-1, b"1 <= n <= 2^32 - 2", n=n, d=0, ld=0)
    refused(-1, b"d >= 1", d=0, ld=0)
    for ld in (2, -1, 0):
        refused(-1, b": ld >= d", ld=ld, m2_ld=0)
    refused(-1, b"does not fit 63 bits", ld=2 ** 62)
    for m2_ld in (2, -1):
        refused(-1, b"m2_ld >= d", m2_ld=m2_ld)
    wide = 64 * 70000                                            # 70000 blocks: 2.45e9 pairs
    refused(-3, b"2^31 - 1", d=wide, ld=wide, m2_ld=wide, ws_bytes=0)
    refused(-4, b"workspace too small", ws_bytes=need - 1)
    for dtype in (0, 1):
        refused(-1, b"must be device memory", dtype=dtype, ws_bytes=need)      # every value is fine
    assert not buf.any()


def test_python_layer_refuses_before_the_device(monkeypatch):
    from d3p_amd import covariance as CV
    monkeypatch.setattr(L, "require_device", lambda: pytest.fail("covariance reached require_device"))
    z = torch.zeros((40, 3))

    def refused(match, fn, *args, **kw):
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)
    for fn in (CV.column_moments, CV.covariance, CV.correlation, lambda t: CV.correlation_fidelity(t, z), lambda t: CV.correlation_fidelity(z, t),
               lambda t: CV.correlation_fidelity(z, z, holdout=t)):
        for bad in (np.zeros((8, 3), np.float32), torch.zeros(()), z[None], z.double(), z.to(torch.int64), torch.zeros((0, 3)), torch.zeros((8, 0))):
            refused("a 2-D float32 or int32 CUDA tensor|at least one row|d >= 1", fn, bad)
        refused("unit stride", fn, torch.zeros((3, 40)).t())
        refused("rows of the tensor overlap", fn, torch.zeros((1, 3)).expand(40, 3))
        refused("CUDA tensor", fn, z)                             # every value is fine; the tensors are the host's
    for ddof in (-1, 40, 1.0, True, None):
        refused("ddof must be an int in", CV.covariance, z, ddof=ddof)
    refused("one dtype for both", CV.correlation_fidelity, z, z.to(torch.int32))
    for kw in (dict(synthetic=torch.zeros((5, 2))), dict(synthetic=z, holdout=torch.zeros((5, 2)))):
        refused("one d for both", CV.correlation_fidelity, z, **kw)
    for top in (-1, 1.5, True, None):
        refused("top must be a non-negative int", CV.correlation_fidelity, z, z, top=top)
