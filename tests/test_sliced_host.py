"""d3p_amd.sliced without a GPU: surface, query functions, refusals in their stated order, directions, the references against each other."""
import ctypes as C

import numpy as np
import pytest
import torch

import d3p_amd._lib as L
from tests import sliced_ref as SR


def test_module_surface_and_geometry():
    import d3p_amd
    from d3p_amd import sliced as SL
    assert d3p_amd.sliced is SL and "sliced" in d3p_amd.__all__
    assert SL.__all__[:5] == ["random_directions", "project", "w2_distance", "sliced_wasserstein", "SlicedWasserstein"]
    assert SL.SlicedWasserstein._fields[:6] == ("sw1", "sw2", "max_w1", "max_w1_at", "max_w2", "max_w2_at") and SL.SlicedWasserstein._fields[-1] == "floor"
    assert "PRIVACY" in SL.__doc__ and "NOT covered by the accountant" in SL.__doc__ and "not covered" in SL.sliced_wasserstein.__doc__
    lib = L.load()
    assert (lib.d3p_project_rows_tile_rows(), lib.d3p_project_rows_chunk_cols(), lib.d3p_project_rows_max_launch_dirs()) == (128, 32, 128)
    assert any(p.endswith("d3p_sliced.hip") for p in L._SRC) and "d3p_sliced.hip" in L._EXTRA_FLAGS


@pytest.mark.parametrize("n_a,n_b,d", [(1, 1, 1), (4096, 3, 3), (4097, 65, 65), (3, 8193, 2), (10 ** 6, 10 ** 5, 64), (2 ** 31 - 1, 1, 1)])
def test_w2_workspace_and_roundings_follow_their_formulas(n_a, n_b, d):
    lib = L.load()
    nblk = -(-max(n_a, n_b) // lib.d3p_sort_columns_block_keys())
    assert lib.d3p_column_w2_distance_workspace(n_a, n_b, d) == lib.d3p_column_w2_distance_workspace(n_b, n_a, d) == 8 * d * nblk
    assert lib.d3p_column_w2_distance_roundings(n_a, n_b) == lib.d3p_column_w2_distance_roundings(n_b, n_a) == 32 + 8 + nblk + 2
    for bad in ((0, 4, 1), (4, 0, 1), (2 ** 31, 4, 1), (4, 4, 0), (2 ** 31 - 1, 1, 2 ** 13)):
        assert lib.d3p_column_w2_distance_workspace(*bad) == 0
    assert lib.d3p_column_w2_distance_roundings(0, 4) == 0 == lib.d3p_column_w2_distance_roundings(4, 2 ** 31)


def test_the_c_entries_refuse_on_the_host_in_the_stated_order():
    lib = L.load()
    buf = np.zeros(8192, np.float32)
    p, odd, odd4 = (C.c_void_p(buf.ctypes.data + k) for k in (0, 2, 4))

    def refused(rc, text, x=p, dtype=0, ld=3, n=40, d=3, theta=p, ld_t=5, dirs=5, shift=p, out=p, ld_p=5):
        assert lib.d3p_project_rows(None, x, dtype, ld, n, d, theta, ld_t, dirs, shift, out, ld_p) == rc and text in lib.d3p_last_error(), text
    for name in ("x", "theta", "out"):
        refused(-1, b"null pointer", **{name: None}, shift=odd)
    for name in ("x", "theta", "shift", "out"):
        refused(-1, b"not aligned to 4 bytes", **{name: odd}, dtype=7)
    refused(-1, b"dtype must be 0 (float32) or 1 (int32)", dtype=2, d=0)
    refused(-1, b"d >= 1", d=0, ld=-1)
    refused(-1, b": ld >= d", ld=2, ld_p=4)
    refused(-1, b"ld_p >= L", ld_p=4, ld_t=4)
    refused(-1, b"ld_t >= L", ld_t=4, n=2 ** 31)
    refused(-1, b"does not fit 63 bits", ld=2 ** 62, n=2 ** 31)
    refused(-3, b"at most 2^31 - 1", n=2 ** 31, shift=None)
    refused(-3, b"more than 2^31 - 1", n=2 ** 31 - 1, dirs=2 ** 20, ld_t=2 ** 20, ld_p=2 ** 20)
    refused(-1, b"must be device memory")                          # every value is fine
    assert lib.d3p_project_rows(None, p, 0, 3, 0, 3, p, 5, 5, None, p, 5) == 0 == lib.d3p_project_rows(None, p, 0, 3, 40, 3, p, 5, 0, None, p, 5)   # nothing to do
    need = lib.d3p_column_w2_distance_workspace(40, 50, 3)

    def refused2(rc, text, a=p, ld_a=40, n_a=40, b=p, ld_b=50, n_b=50, dtype=0, d=3, out=p, ws=p, ws_bytes=1 << 20):
        assert lib.d3p_column_w2_distance(None, a, ld_a, n_a, b, ld_b, n_b, dtype, d, out, ws, ws_bytes) == rc and text in lib.d3p_last_error(), text
    for name in ("a", "b", "out", "ws"):
        refused2(-1, b"null pointer", **{name: None}, dtype=9)
    refused2(-1, b"not aligned to 4 bytes", a=odd, out=odd4)
    refused2(-1, b"not aligned to 8 bytes", out=odd4, dtype=9)
    refused2(-1, b"dtype must be", dtype=9, n_a=0)
    refused2(-1, b"1 <= n_a, n_b <= 2^31 - 1", n_b=2 ** 31, d=0)
    refused2(-1, b"d >= 1", d=0, ld_a=0)
    refused2(-1, b"ld_a >= n_a and ld_b >= n_b", ld_b=49, ws_bytes=0)
    refused2(-1, b"does not fit 63 bits", ld_a=2 ** 62, ws_bytes=0)
    refused2(-3, b"more than 2^31 - 1", n_a=2 ** 31 - 1, ld_a=2 ** 31, d=2 ** 13, ws_bytes=0)
    refused2(-4, b"workspace too small", ws_bytes=need - 1)
    refused2(-1, b"must be device memory", ws_bytes=need)
    assert not buf.any()


def test_python_layer_refuses_before_the_device(monkeypatch):
    from d3p_amd import sliced as SL
    monkeypatch.setattr(L, "require_device", lambda: pytest.fail("sliced reached require_device"))
    z, th, s = torch.zeros((40, 3)), torch.zeros((3, 5)), torch.zeros((3, 40))
    cases = [("d >= 1", SL.project, (torch.zeros((8, 0)), th), {}), ("unit stride", SL.sliced_wasserstein, (z, torch.zeros((3, 40)).t()), {}),
             ("CUDA tensor", SL.project, (z, th), {}), ("CUDA tensor", SL.sliced_wasserstein, (z, z), {"holdout": z}),
             ("theta", SL.project, (z, torch.zeros((2, 5))), {}),
             ("shift must be None or a contiguous float32", SL.project, (z, th, torch.zeros(6)[::2]), {}),
             ("one d for both", SL.sliced_wasserstein, (z, torch.zeros((5, 2))), {}), ("must be an int >=", SL.sliced_wasserstein, (z, z), {"n_dirs": 0}),
             ("scale must be None or a floating-point tensor", SL.sliced_wasserstein, (z, z), {"scale": "iqr"}),
             ("sa: ", SL.w2_distance, (s[0], s), {}), ("one dtype for both", SL.w2_distance, (s, s.to(torch.int32)), {}),
             ("CUDA tensor", SL.w2_distance, (s, s), {})]
    for match, fn, args, kw in cases:
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)


def test_random_directions_are_unit_and_independent_of_the_slab():
    from d3p_amd import sliced as SL
    theta = SL.random_directions(7, 40, seed=3)
    assert theta.shape == (7, 40) and theta.dtype == torch.float32 and not theta.is_cuda
    assert np.abs(theta.double().norm(dim=0).numpy() - 1.0).max() <= 7 * SR.U32          # one float32 rounding per entry
    assert torch.equal(SL.random_directions(7, 9, seed=3), theta[:, :9])                   # direction l is a function of (seed, d, l)
    scaled = SL.random_directions(7, 40, seed=3, scale=torch.tensor([2.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.5]))
    assert not scaled[1].any() and torch.equal(scaled[0], 2.0 * theta[0]) and not torch.equal(SL.random_directions(7, 9, seed=4), theta[:, :9])


@pytest.mark.parametrize("n_a,n_b", [(1, 1), (1, 5), (5, 1), (7, 7), (7, 5), (4, 9), (12, 8), (13, 31)])
def test_the_references_agree_with_each_other(n_a, n_b):
    r = np.random.default_rng(n_a * 37 + n_b)
    a, b = np.sort(r.normal(size=n_a).astype(np.float32)), np.sort(r.normal(1.0, 2.0, size=n_b).astype(np.float32))
    for p in (1, 2):
        got, brute = SR.wasserstein(a, b, p)[0], SR.wasserstein_brute(a, b, p)
        assert abs(got - brute) <= 8 * SR.U64 * brute and SR.wasserstein(b, a, p)[0] == got
        assert SR.wasserstein(a, a, p)[0] == 0.0
    if n_a == n_b:
        closed = float(np.sum((a.astype(np.float64) - b.astype(np.float64)) ** 2)) / n_a
        assert abs(SR.wasserstein(a, b, 2)[0] - closed) <= (n_a + 4) * SR.U64 * closed
