"""The two-site guide kind of the run loop (D3P_GUIDE_EXP_SITES) at the C-ABI boundary, without a GPU: the name in the header and in
_lib, the unchanged ABI version, and every entry point that does not run it refusing it before it touches the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import d3p_amd._lib as L
    L.build()
    return L, L.load()


def test_the_new_guide_kind_is_named_in_the_header_and_in_python():
    import d3p_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "d3p_hip.h")).read()
    m = re.search(r"#define D3P_GUIDE_EXP_SITES (\d+)", hdr)
    assert m and int(m.group(1)) == L.D3P_GUIDE_EXP_SITES == 2
    assert L.D3P_GUIDE_SOFTPLUS == 0 and L.D3P_GUIDE_EXP == 1
    _, lib = _lib()
    assert lib.d3p_abi_version() == 9


def _args(L, guide, d=16, B=32, N=1000):
    m = L.LogregModel(d, 1, 1.0, 2.0, float(N), 1.0 / N, L.D3P_FAMILY_LOGREG, guide, 0.0)
    h = L.DpsviHyper(1.0, 0.5, 1e-2, 0.9, 0.999, 1e-8)
    fake = ctypes.c_void_p(0x1000)   # (never dereferenced: the refusal comes first)
    st = L.DpsviState(fake.value, 0, fake.value, fake.value, fake.value, fake.value)
    src = L.BatchSource(L.D3P_BATCH_FEISTEL, B, 0.0, 0, fake.value, fake.value, None, N, 0, N)
    return m, h, st, src, fake


# every entry point that takes a logreg model and does device work, except the single-GPU runs
_REFUSING = ["d3p_logreg_evaluate", "d3p_logreg_evaluate_sites", "d3p_logreg_evaluate_particles", "d3p_logreg_evaluate_sites_particles",
             "d3p_logreg_px_grads", "d3p_logreg_px_grads_particles", "d3p_dpvi_logreg_local_sums", "d3p_dpvi_logreg_local_sums_particles",
             "d3p_dpvi_logreg_finalize", "d3p_dpvi_logreg_begin", "d3p_dpvi_logreg_prepare", "d3p_dpvi_logreg_step_sums",
             "d3p_dpvi_logreg_step_finalize", "d3p_dpvi_logreg_end", "d3p_dpvi_logreg_prepare_buf", "d3p_dpvi_logreg_acc_reset",
             "d3p_dpvi_logreg_fused_step", "d3p_dpvi_logreg_run_xchg", "d3p_dpvi_logreg_run_dist_from", "d3p_dpvi_logreg_time_main_kernel"]


@pytest.mark.parametrize("name", _REFUSING)
def test_entry_points_that_do_not_run_it_refuse_it_first(name):
    """Called with the new kind and otherwise plausible arguments (pointers to a zeroed host buffer, counts of 2), each refuses with
    D3P_E_UNSUPPORTED and names the kind -- before any launch: without a GPU a launch would fail with D3P_E_HIP instead."""
    L, lib = _lib()
    m, h, st, src, _ = _args(L, L.D3P_GUIDE_EXP_SITES)
    host = (ctypes.c_uint8 * (1 << 20))()
    fake = ctypes.addressof(host)
    st = L.DpsviState(fake, 0, fake, fake, fake, fake)
    src = L.BatchSource(L.D3P_BATCH_FEISTEL, 32, 0.0, 0, fake, fake, None, 1000, 0, 1000)
    ws = lib.d3p_dpvi_logreg_workspace(ctypes.byref(m), ctypes.byref(src))
    _, argtypes = L.SIGNATURES[name]
    args = []
    for t in argtypes:
        if t is L._PM:
            args.append(ctypes.byref(m))
        elif t is L._PH:
            args.append(ctypes.byref(h))
        elif t is L._PS:
            args.append(ctypes.byref(st))
        elif t is L._PB:
            args.append(ctypes.byref(src))
        elif t is L._SZ:
            args.append(ws)
        elif t is L._V:
            args.append(fake)
        elif isinstance(t, type) and issubclass(t, ctypes._Pointer):
            args.append(ctypes.cast(fake, t))
        else:
            args.append(2)
    if name == "d3p_dpvi_logreg_run_dist_from":
        args[1] = None   # (one of comm / xchg)
    assert getattr(lib, name)(*args) == -3, (name, lib.d3p_last_error())   # D3P_E_UNSUPPORTED
    assert b"D3P_GUIDE_EXP_SITES" in lib.d3p_last_error(), (name, lib.d3p_last_error())


def test_the_run_entry_points_take_it_past_validation():
    """d3p_dpvi_logreg_run_from does not refuse the kind itself: with a null data pointer it fails on that instead."""
    L, lib = _lib()
    m, h, st, src, fake = _args(L, L.D3P_GUIDE_EXP_SITES)
    B = ctypes.byref
    ws = lib.d3p_dpvi_logreg_workspace(B(m), B(src))
    rc = lib.d3p_dpvi_logreg_run_from(None, B(m), B(h), B(st), B(st), B(src), 0, None, fake, 1, fake, fake, ws)
    assert rc < 0
    assert b"D3P_GUIDE_EXP_SITES" not in lib.d3p_last_error()


def test_the_kind_needs_an_intercept():
    L, lib = _lib()
    m, h, st, src, fake = _args(L, L.D3P_GUIDE_EXP_SITES)
    m.intercept = 0
    B = ctypes.byref
    ws = lib.d3p_dpvi_logreg_workspace(B(m), B(src))
    rc = lib.d3p_dpvi_logreg_run_from(None, B(m), B(h), B(st), B(st), B(src), 0, fake, fake, 1, fake, fake, ws)
    assert rc < 0 and b"intercept" in lib.d3p_last_error()


def test_the_workspace_grows_only_for_the_new_kind():
    L, lib = _lib()
    m1, _, _, src, _ = _args(L, L.D3P_GUIDE_EXP)
    m2, _, _, _, _ = _args(L, L.D3P_GUIDE_EXP_SITES)
    B = ctypes.byref
    a, b = lib.d3p_dpvi_logreg_workspace(B(m1), B(src)), lib.d3p_dpvi_logreg_workspace(B(m2), B(src))
    assert b >= a + 2 * 128 * 32 * 4


@pytest.mark.parametrize("name,extra", [("d3p_dpvi_logreg_run_from", ()), ("d3p_dpvi_logreg_run", ())])
def test_the_run_entry_points_refuse_rows_too_wide_for_the_fused_step(name, extra):
    """d + 1 > 1024: the two-kernel steps have no two-site form; refused before any launch (run_steps asks first and walks stepwise)."""
    L, lib = _lib()
    m, h, st, src, _ = _args(L, L.D3P_GUIDE_EXP_SITES, d=1024)
    host = (ctypes.c_uint8 * (1 << 20))()
    fake = ctypes.addressof(host)
    B = ctypes.byref
    ws = lib.d3p_dpvi_logreg_workspace(B(m), B(src))
    st = L.DpsviState(fake, 0, fake, fake, fake, fake)
    src = L.BatchSource(L.D3P_BATCH_FEISTEL, 32, 0.0, 0, fake, fake, None, 1000, 0, 1000)
    assert not lib.d3p_dpvi_logreg_fused_step_supported(B(m), B(src))
    if name == "d3p_dpvi_logreg_run_from":
        st2 = L.DpsviState(fake + 4096, 0, fake + 65536, fake + 131072, fake + 196608, fake + 8192)
        rc = lib.d3p_dpvi_logreg_run_from(None, B(m), B(h), B(st2), B(st), B(src), 0, fake, fake, 1, fake, fake, ws)
    else:
        rc = lib.d3p_dpvi_logreg_run(None, B(m), B(h), B(st), B(src), fake, fake, 1, fake, fake, ws)
    assert rc == -3 and b"fused step only" in lib.d3p_last_error(), lib.d3p_last_error()


def test_run_from_refuses_a_state_that_aliases_its_source():
    L, lib = _lib()
    m, h, st, src, _ = _args(L, L.D3P_GUIDE_EXP_SITES)
    host = (ctypes.c_uint8 * (1 << 20))()
    fake = ctypes.addressof(host)
    B = ctypes.byref
    st = L.DpsviState(fake, 0, fake + 4096, fake + 8192, fake + 12288, fake)
    src = L.BatchSource(L.D3P_BATCH_FEISTEL, 32, 0.0, 0, fake, fake, None, 1000, 0, 1000)
    ws = lib.d3p_dpvi_logreg_workspace(B(m), B(src))
    rc = lib.d3p_dpvi_logreg_run_from(None, B(m), B(h), B(st), B(st), B(src), 0, fake, fake, 1, fake, fake, ws)
    assert rc == -1 and b"apart from" in lib.d3p_last_error(), lib.d3p_last_error()
