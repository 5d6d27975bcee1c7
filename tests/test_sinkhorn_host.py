"""d3p_amd.sinkhorn without a GPU: surface and signatures, the reference against its own bound, the GPU table's inputs, the dense
reference iteration on cases with a known answer, refusals before the device."""
import os
import re

import numpy as np
import pytest
import torch

import d3p_amd._lib as L
from tests import sinkhorn_ref as SR
from tests import test_gpu_sinkhorn as G
from tests.test_gpu_mmd import table

ARITY = {"d3p_softmin_rows": 20, "d3p_softmin_rows_workspace": 2, "d3p_softmin_rows_group_tiles": 0, "d3p_softmin_rows_resident_cols": 0,
         "d3p_softmin_rows_segments": 2, "d3p_softmin_rows_segment_tiles": 2, "d3p_softmin_rows_roundings": 2, "d3p_softmin_rows_set_segments": 1}


def test_surface_declaration_and_geometry():
    import d3p_amd
    from d3p_amd import sinkhorn as S
    assert d3p_amd.sinkhorn is S and "sinkhorn" in d3p_amd.__all__ and S.__all__[:3] == ["softmin_rows", "sinkhorn_divergence", "SinkhornDivergence"]
    assert S.SinkhornDivergence._fields[:8] == ("divergence", "ot_xy", "f_x", "g_y", "epsilon", "n_iter_run", "converged", "marginal_error")
    assert "PRIVACY" in S.__doc__ and "NOT covered by the accountant" in S.__doc__ and "not covered" in S.sinkhorn_divergence.__doc__
    with open(os.path.join(os.path.dirname(os.path.dirname(L.__file__)), "include", "d3p_hip.h")) as f:
        hdr = f.read()
    lib = L.load()
    assert lib.d3p_abi_version() == 9
    for name, n in ARITY.items():
        args = re.search(r"^(?:int|size_t|uint32_t) " + name + r"\(([^)]*)\)", hdr, re.M).group(1).strip()
        assert (0 if args == "void" else args.count(",") + 1) == n == len(L.SIGNATURES[name][1]) and hasattr(lib, name), name
    assert any(p.endswith("d3p_sinkhorn.hip") for p in L._SRC) and any(p.endswith("d3p_gram_tile.h") for p in L._DEPS)
    assert (lib.d3p_softmin_rows_group_tiles(), lib.d3p_softmin_rows_resident_cols()) == (64, 64)
    assert lib.d3p_softmin_rows_workspace(40, 50) == lib.d3p_softmin_rows_segments(40, 50) * 40 * 20 + 4 * 90
    assert lib.d3p_softmin_rows_workspace(0, 4) == 0 and lib.d3p_softmin_rows_set_segments(-1) == -1 and b"segments must be 0" in lib.d3p_last_error()
    # refused on the host, before any launch: h is required; omega lies in (0, 1]; logw and out_h come together
    buf = np.zeros(4096, np.float32)
    p, need = L.C.c_void_p(buf.ctypes.data), lib.d3p_softmin_rows_workspace(40, 50)
    for text, kw in ((b"null pointer", {"h": None}), (b"gamma must be finite and > 0", {"gamma": 0.0}), (b"omega must be in (0, 1]", {"omega": 1.5}),
                     (b"given together", {"out_h": None}), (b"workspace too small", {"ws_bytes": need - 1}), (b"must be device memory", {})):
        a = {"h": p, "gamma": 0.5, "omega": 1.0, "out_h": p, "ws_bytes": need, **kw}
        assert lib.d3p_softmin_rows(None, p, p, 0, 3, 3, 40, 50, 3, p, p, a["gamma"], a["h"], p, a["omega"], p, p, a["out_h"], p, a["ws_bytes"]) < 0
        assert text in lib.d3p_last_error(), text


def test_the_reference_passes_its_own_bound_on_an_uncentred_table_only_with_the_shift():
    """Columns at 10^4 +- 1: the rule in float32 numpy is within the bound of the float64 reference with the shift, and the Gram form
    without it is not."""
    a, b = table(40, 5, False, 1), table(50, 5, False, 2)
    h, shift = np.random.default_rng(3).normal(size=50).astype(np.float32), b.astype(np.float64).mean(axis=0).astype(np.float32)
    bound_shifted = SR.softmin_rows(a, b, 0.7, h, shift)[1]
    for sh, inside in ((shift, True), (None, False)):
        want, bound = SR.softmin_rows(a, b, 0.7, h, sh)
        err = np.abs(SR.softmin_f32(a, b, 0.7, h, sh) - want)
        assert bool((err <= bound).all()) and bool((err <= bound_shifted).all()) == inside


@pytest.mark.parametrize("na,nb,d,is_int,stride,given,segments,with_prev,with_logw", G.CASES)
def test_the_bound_of_every_gpu_case_is_not_vacuous(na, nb, d, is_int, stride, given, segments, with_prev, with_logw):
    """A condition on the inputs of the GPU table: the reference's bound on L stays below a hundredth of a bit."""
    a, b, shift, scale, gamma, h = G.inputs(na, nb, d, is_int, given, with_prev, with_logw)[:6]
    assert float(SR.softmin_rows(a, b, gamma, h, shift, scale, None, 1.0, None, 64)[1].max()) < 0.01


def test_the_dense_reference_on_cases_with_a_known_answer():
    x, y = table(12, 3, False, 4, 0.0), table(9, 3, False, 5, 0.0)
    div, ot = SR.sinkhorn(x[:1], y[:1], 0.3, np.ones(1), np.ones(1), rungs=(3.0, 0.75), n_iter=5)[:2]
    cost = 0.5 * float(((x[:1].astype(np.float64) - y[:1]) ** 2).sum())
    assert abs(div - cost) < 8 * SR.U32 * cost and abs(ot - cost) < 8 * SR.U32 * cost          # (gamma and h are float32: a few u of the cost)
    assert abs(SR.sinkhorn(x, x, 0.3, np.ones(12), np.ones(12), rungs=(3.0,), n_iter=5)[0]) < 1e-12
    assert SR.sinkhorn(x, y, 0.3, np.ones(12), np.ones(9), n_iter=5)[0] > 0.0                      # a divergence of two different tables


def test_python_layer_refuses_before_the_device(monkeypatch):
    from d3p_amd import sinkhorn as S
    monkeypatch.setattr(L, "require_device", lambda: pytest.fail("sinkhorn reached require_device"))
    z, zi, h = torch.zeros((40, 3)), torch.zeros((40, 3), dtype=torch.int32), torch.zeros(40)
    sd, sr = S.sinkhorn_divergence, S.softmin_rows
    cases = [("d >= 1", sr, (torch.zeros((8, 0)), z, 1.0, h), {}), ("unit stride", sd, (z, torch.zeros((3, 40)).t()), {}),
             ("one dtype for both", sr, (z, zi, 1.0, h), {}), ("one d for both", sd, (z, torch.zeros((5, 2))), {}),
             ("gamma must be a finite number > 0", sr, (z, z, 0.0, h), {}), ("h must be a contiguous float32", sr, (z, z, 1.0, h[:39]), {}),
             ("shift must be None or a contiguous float32", sr, (z, z, 1.0, h), {"shift": torch.zeros(6)[::2]}),
             ("prev must be None or a contiguous float64", sr, (z, z, 1.0, h), {"prev": h}), ("omega must be a number in", sr, (z, z, 1.0, h), {"omega": 0.0}),
             ("logw must be None or a contiguous float32", sr, (z, z, 1.0, h), {"logw": h.double()}),
             ("epsilon must be 'median' or", sd, (z, z), {"epsilon": "mean"}), ("epsilon must be a finite", sd, (z, z), {"epsilon": -1.0}),
             ("epsilon_share must be", sd, (z, z), {"epsilon_share": 0.0}), ("wx must be None or a floating", sd, (z, z), {"wx": torch.ones(39)}),
             ("n_iter must be an int >= 1", sd, (z, z), {"n_iter": 0}), ("check_every must be", sd, (z, z), {"check_every": 1.5}),
             ("tol must be", sd, (z, z), {"tol": 0.0}), ("scaling must be a number in", sd, (z, z), {"scaling": 1.0}),
             ("scale must be 'std' or None", sd, (z, z), {"scale": "iqr"}), ("CUDA tensor", sr, (z, z, 1.0, h), {}), ("CUDA tensor", sd, (z, z), {})]
    for match, fn, args, kw in cases:
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)
