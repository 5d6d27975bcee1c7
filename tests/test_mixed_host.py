"""Mixed-type pair statistics without a GPU: the restatement of tests/mixed_ref.py against float64 within the bound its header derives,
the entry's refusals in their order (they run before any launch) and the Python layer's host checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import mixed_ref as MR

SPLITS = ((0, 1), (1, 0), (3, 5), (4, 4), (5, 129), (33, 3))


def kinds(dn, dc, seed=0):   # dn numeric and dc categorical columns, interleaved
    return np.random.default_rng(seed).permutation(np.array([0] * dn + [1] * dc)).tolist()


@pytest.mark.parametrize("dn,dc", SPLITS)
@pytest.mark.parametrize("is_int", (False, True), ids=("float32", "int32"))
def test_restatement_lies_within_the_derived_bound(dn, dc, is_int):
    kind = kinds(dn, dc)
    scale, w = MR.schema(5, kind)
    a, b = MR.data(1, 37, kind, is_int), MR.data(2, 41, kind, is_int)
    em, ex = MR.emulate(a, b, kind, scale, w), MR.exact(a, b, kind, scale, w)
    err, tol = np.abs(em["dist"].astype(np.float64) - ex["dist"]), MR.gamma(2 * dn + 1, MR.U32) * ex["dist"]
    assert (err <= tol).all(), float((err / tol).max())
    # the single rounding: w_cat * m + qn is exact in float64 on these inputs (all of them multiples of 2^-20 below 2^20)
    assert (np.ldexp(ex["dist"], 20) == np.round(np.ldexp(ex["dist"], 20))).all() and ex["dist"].max() < 2.0 ** 20
    if dn == 0:
        assert np.array_equal(em["dist"].astype(np.float64), ex["dist"])            # 0.75 m: exact
    print(f"({dn}, {dc}) largest error / bound {float((err[tol > 0] / tol[tol > 0]).max()):.3f}")


def test_entry_refusals_run_in_order_before_any_launch():
    import d3p_amd._lib as L
    lib = L.load()
    assert [int(lib.d3p_pair_mixed_packed_words(dn, dc)) for dn, dc in SPLITS] == [1, 4, 6, 5, 41, 37]
    assert lib.d3p_pair_stats_mixed_segment_tiles() == 16 and lib.d3p_pair_stats_mixed_roundings(513) == 16 + 3 + 4 + 2
    assert lib.d3p_pair_stats_mixed_form(0, 1, 1) == 0 and lib.d3p_pair_stats_mixed_workspace(0, 1, 1, 0) == 0
    need = int(lib.d3p_pair_stats_mixed_workspace(4, 4, 1, 1))
    assert need == 8 * (2 + 3 + 3) + 2 * 4 * 4 * 5 + 2 * 4 * 4                  # positions, two packed tables of 5 words, flags
    buf = np.zeros(64, np.float64)                                                # host memory: never reaches a kernel
    p = buf.ctypes.data

    def call(kind=(0, 1), scale=(1.0, 0.0), w=1.0, excl=0, ws=need, d=2, a=p):
        k, s = (C.c_uint8 * 2)(*kind), (C.c_float * 2)(*scale)
        rc = lib.d3p_pair_stats_mixed(None, a, p, 0, 2, 2, 4, 4, d, C.cast(k, C.c_void_p), C.cast(s, C.c_void_p), w, excl, p, p, p, p, ws)
        return rc, lib.d3p_last_error().decode()
    for args, rc, text in (({"a": None}, -1, "null pointer"), ({"a": p + 2}, -1, "aligned to 4"), ({"d": 0, "kind": (2, 0)}, -1, "d >= 1"),
                           ({"kind": (0, 2), "scale": (-1.0, 0.0)}, -1, "kind[1]"), ({"scale": (-1.0, 0.0), "w": -1.0}, -1, "scale[0]"),
                           ({"scale": (float("inf"), 0.0)}, -1, "scale[0]"), ({"scale": (1.0, float("nan"))}, -1, "device memory"),
                           ({"w": float("nan"), "excl": 2}, -1, "w_cat"), ({"w": -0.5}, -1, "w_cat"), ({"excl": 2, "ws": 0}, -1, "exclude_diagonal"),
                           ({"ws": need - 1}, -4, "workspace too small"), ({}, -1, "device memory")):
        got = call(**args)
        assert got[0] == rc and text in got[1], (args, got)
    assert lib.d3p_pair_stats_mixed_set_form(3) == -1 and lib.d3p_pair_stats_mixed_set_form(0) == 0


def test_python_host_checks_run_before_the_device():
    from d3p_amd import fidelity as F
    from d3p_amd import mixed as M
    real, a, b = torch.zeros((8, 3)), torch.zeros((8, 3)), torch.zeros((5, 3))
    for cats, w, text in (((3,), None, "outside"), ((1, 1), None, "distinct"), ((0.5,), None, "sequence"), ((1,), (1, -1, 1), "weights"),
                          ((1, 2), (1, 1, 2), "share one weight"), ((1,), None, "CUDA tensor")):
        with pytest.raises(ValueError, match=text):
            M.mixed_schema(real, cats, w)
    schema = M.MixedSchema((0, 1, 0), (0.125, 0.0, 0.0), 0.75, 2.75, (8.0, float("nan"), 0.0))
    for fn in (M.pair_stats, M.energy_distance, M.closest_record, lambda x, y, s: F.fidelity_report(x, y, schema=s)):
        for x, y, s, text in ((a, b.to(torch.int32), schema, "one dtype for both"), (a, b, (0, 1, 0), "MixedSchema"),
                              (a[:, :2], b[:, :2], schema, "the schema has 3 columns and the tables 2"),
                              (a, b, schema._replace(w_cat=-1.0), "finite and >= 0"), (a, b, schema, "CUDA tensor")):
            with pytest.raises(ValueError, match=text):
                fn(x, y, s)
