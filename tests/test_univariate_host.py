"""d3p_amd.univariate without a GPU: the surface, the arithmetic of the query functions, the refusals of the C entries and of the Python
layer, and where the kernels are compiled."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import d3p_amd._lib as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "d3p_amd", "csrc")


def test_module_surface():
    import d3p_amd
    from d3p_amd import univariate as UV
    assert d3p_amd.univariate is UV and "univariate" in d3p_amd.__all__
    assert UV.__all__ == ["sort_columns", "midranks", "spearman", "cdf_distance", "univariate_fidelity", "CdfDistance", "UnivariateFidelity", "INT_EXACT"]
    assert UV.CdfDistance._fields[:5] == ("ks", "ks_at", "w1", "n_a", "n_b")
    assert "PRIVACY" in UV.__doc__ and "NOT covered by the accountant" in UV.__doc__ and "not covered" in UV.univariate_fidelity.__doc__


@pytest.mark.parametrize("n,d", [(1, 1), (4096, 3), (4097, 65), (8192, 2), (8193, 2), (20001, 5), (10 ** 6, 64), (2 ** 31 - 1, 1)])
def test_query_functions_give_the_geometry(n, d):
    lib = L.load()
    T, stage = lib.d3p_sort_columns_block_keys(), lib.d3p_sort_columns_staged_keys()
    assert (T, stage) == (4096, 8192)
    nblk = -(-n // T)
    assert lib.d3p_sort_columns_rank_stride(n) == -(-n // stage)
    assert lib.d3p_sort_columns_workspace(n, d, 0) == 4 * (2 * n * d + 256 * nblk * d)
    assert lib.d3p_sort_columns_workspace(n, d, 1) == (lib.d3p_sort_columns_workspace(n, d, 0) if n < 2 ** 30 else 0)
    assert lib.d3p_column_cdf_distance_workspace(n, 5000, d) == -(-20 * d * (nblk + 2) // 8) * 8
    assert lib.d3p_column_cdf_distance_roundings(n, 5000) == 5 + 16 + 8 + nblk + 2
    for bad in ((0, 4), (4, 0), (2 ** 31, 4), (2 ** 31 - 1, 2 ** 13)):
        assert lib.d3p_sort_columns_workspace(*bad, 0) == 0 and lib.d3p_column_cdf_distance_workspace(bad[0], 7, bad[1]) == 0


def test_the_c_entries_refuse_on_the_host_as_declared():
    lib = L.load()
    buf = np.zeros(8192, np.float32)
    p, odd, odd4 = (C.c_void_p(buf.ctypes.data + k) for k in (0, 2, 4))
    need = lib.d3p_sort_columns_workspace(40, 3, 1)

    def refused(rc, text, x=p, dtype=0, ld=3, n=40, d=3, out=p, ld_s=40, ranks=p, ld_r=3, ws=p, ws_bytes=1 << 20):
        assert lib.d3p_sort_columns(None, x, dtype, ld, n, d, out, ld_s, ranks, ld_r, ws, ws_bytes) == rc and text in lib.d3p_last_error(), text
    for name in ("x", "out", "ws"):
        refused(-1, b"null pointer", **{name: None})
    for name in ("x", "out", "ranks", "ws"):
        refused(-1, b"not aligned to 4 bytes", **{name: odd})
    refused(-1, b"null pointer", x=None, out=odd)                 # the order: null, alignment, dtype, n, d, ld, ld_s, ld_r, 63 bits, grid, workspace
    refused(-1, b"not aligned", x=odd, dtype=7)
    refused(-1, b"dtype must be 0 (float32) or 1 (int32)", dtype=2, n=0)
    for n in (0, 2 ** 31, 2 ** 40):
        refused(-1, b"1 <= n <= 2^31 - 1", n=n, d=0)
    refused(-1, b"n <= 2^30 - 1", n=2 ** 30, d=0)
    refused(-1, b"d >= 1", d=0, ld=0)
    refused(-1, b": ld >= d", ld=2, ld_s=0)
    refused(-1, b"ld_s >= n", ld_s=39, ld_r=0)
    refused(-1, b"ld_r >= d", ld_r=2)
    refused(-1, b"does not fit 63 bits", ld=2 ** 62)
    refused(-3, b"2^31 - 1", n=2 ** 31 - 1, ld_s=2 ** 31, d=2 ** 13, ld=2 ** 13, ranks=None, ws_bytes=0)
    refused(-4, b"workspace too small", ws_bytes=need - 1)
    refused(-1, b"must be device memory", ws_bytes=need)         # every value is fine
    need = lib.d3p_column_cdf_distance_workspace(40, 50, 3)

    def refused2(rc, text, a=p, ld_a=40, n_a=40, b=p, ld_b=50, n_b=50, dtype=0, d=3, num=p, at=p, w1=p, ws=p, ws_bytes=1 << 20):
        assert lib.d3p_column_cdf_distance(None, a, ld_a, n_a, b, ld_b, n_b, dtype, d, num, at, w1, ws, ws_bytes) == rc and text in lib.d3p_last_error(), text
    for name in ("a", "b", "num", "at", "w1", "ws"):
        refused2(-1, b"null pointer", **{name: None})
    refused2(-1, b"not aligned to 4 bytes", a=odd, dtype=9)
    refused2(-1, b"not aligned to 8 bytes", w1=odd4, dtype=9)
    refused2(-1, b"dtype must be", dtype=9, n_a=0)
    refused2(-1, b"1 <= n_a, n_b <= 2^31 - 1", n_b=2 ** 31, d=0)
    refused2(-1, b"d >= 1", d=0, ld_a=0)
    refused2(-1, b"ld_a >= n_a and ld_b >= n_b", ld_b=49)
    refused2(-4, b"workspace too small", ws_bytes=need - 1)
    refused2(-1, b"must be device memory", ws_bytes=need)
    assert not buf.any()


def test_python_layer_refuses_before_the_device(monkeypatch):
    from d3p_amd import univariate as UV
    monkeypatch.setattr(L, "require_device", lambda: pytest.fail("univariate reached require_device"))
    z = torch.zeros((40, 3))

    def refused(match, fn, *args, **kw):
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)
    for fn in (UV.sort_columns, UV.midranks, UV.spearman, lambda t: UV.cdf_distance(t, z), lambda t: UV.cdf_distance(z, t),
               lambda t: UV.univariate_fidelity(z, t), lambda t: UV.univariate_fidelity(z, z, holdout=t)):
        for bad in (np.zeros((8, 3), np.float32), z[None], z.double(), torch.zeros((0, 3)), torch.zeros((8, 0))):
            refused("a 2-D float32 or int32 CUDA tensor|at least one row|d >= 1", fn, bad)
        refused("unit stride", fn, torch.zeros((3, 40)).t())
        refused("CUDA tensor", fn, z)                             # every value is fine; the tensors are the host's
    big = torch.empty(2 ** 23 + 1)                                # 2 n > 2^24 (never read)
    for fn in (UV.spearman, lambda t: UV.univariate_fidelity(t, t)):
        refused("beyond 2\\^24 in magnitude", fn, big)
    refused("one dtype for both", UV.cdf_distance, z, z.to(torch.int32))
    refused("one d for both", UV.univariate_fidelity, z, torch.zeros((5, 2)))
    for top in (-1, 1.5, True, None):
        refused("top must be a non-negative int", UV.univariate_fidelity, z, z, top=top)


def test_the_kernels_are_compiled_behind_the_order_keys_by_one_existing_user():
    texts = {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC))}
    users = [name for name, text in texts.items() if '#include "d3p_colsort_global_kernel.h"' in text]
    assert users == ["d3p_quantiles.hip"]
    text = texts[users[0]]
    assert text.index('#include "d3p_colreduce.h"') < text.index('#include "d3p_colsort_global_kernel.h"')
    host = texts["d3p_sort_columns.hip"]
    assert re.findall(r'#include\s+"([^"]+)"', host) == ["d3p_sort_columns.h"] and "key_of" not in host and "extern __shared__" not in texts["d3p_colsort_global_kernel.h"]
