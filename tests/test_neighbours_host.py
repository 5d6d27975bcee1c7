"""d3p_amd.neighbours without a GPU: the module surface and its lazy import, the query functions and the bounded workspace, and every
refusal of the C entry and of the Python layer before the device is touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20


@pytest.fixture
def lib():
    import d3p_amd._lib as L
    lib = L.load()
    yield lib
    assert lib.d3p_pair_knn_set_form(0) == 0


def test_module_surface_and_lazy_import():
    import d3p_amd
    from d3p_amd import neighbours as N
    names = d3p_amd.__all__
    assert d3p_amd.neighbours is N and names.index("neighbours") + 1 == names.index("covariance")
    assert N.__all__ == ["knn", "kth_neighbour", "ball_counts", "prdc", "max_k", "PRDC", "INT_EXACT"]
    assert N.PRDC._fields == ("precision", "recall", "density", "coverage", "authenticity", "k", "n_real", "n_synthetic", "dim", "floor")
    assert "PRIVATE" in N.__doc__ and "NOT covered by the accountant" in N.__doc__ and "not covered" in N.prdc.__doc__
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.neighbours' not in sys.modules; " \
           "d3p_amd.neighbours; assert 'd3p_amd.neighbours' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_query_functions_and_the_bounded_workspace(lib):
    T, KMAX = lib.d3p_pair_knn_tile_rows(), lib.d3p_pair_knn_max_k()
    assert KMAX >= 16 and KMAX == __import__("d3p_amd").neighbours.max_k()
    assert [lib.d3p_pair_knn_capacity(k) for k in (0, 1, 2, 4, 5, 8, 9, KMAX, KMAX + 1)] == [0, 1, 4, 4, 8, 8, 16, 16, 0]
    big = ((10 ** 6, 10 ** 6, 784, KMAX), (33, 2 ** 32 - 2, 1, KMAX))
    for forced in (0, 1, 2):
        assert lib.d3p_pair_knn_set_form(forced) == 0
        for na, nb, d, k in big + ((1, 1, 1, 1), (2048, 2048, 2, 5), (4096 * T, 10 ** 6, 3, KMAX), (4096 * T + 1, 10 ** 6, 3, KMAX)):
            form, need, G = lib.d3p_pair_knn_form(na, nb, d, k), lib.d3p_pair_knn_workspace(na, nb, d, k), lib.d3p_pair_knn_segment_tiles(na, nb, d, k)
            assert form in (1, 2) and (forced == 0 or form == forced or na > 4096 * T) and need <= 64 * MIB and G >= 4 and G % 4 == 0
            segments = -(-(-(-nb // T)) // G)
            assert need == (0 if form == 1 else segments * na * (8 * k + 8)) and segments * -(-na // T) <= 4096 + -(-na // T)
    assert lib.d3p_pair_knn_set_form(0) == 0
    assert lib.d3p_pair_knn_form(*big[0]) == 1 and lib.d3p_pair_knn_form(*big[1]) == 2      # the tiles of a fill the chip / cannot
    assert lib.d3p_pair_knn_form(2048, 2048, 2, 5) == 2 and lib.d3p_pair_knn_form(2048, 16 * T, 2, 5) == 1      # one segment: nothing to deal out
    assert lib.d3p_pair_knn_form(4, 4, 2, KMAX + 1) == 0 and lib.d3p_pair_knn_workspace(0, 4, 2, 1) == 0
    assert lib.d3p_pair_knn_set_form(3) == -1 and b"form must be" in lib.d3p_last_error()


def test_the_c_entry_refuses_on_the_host_as_declared(lib):
    buf = np.zeros(8192, np.float32)              # (host memory, never reached)
    p, odd, odd4 = (C.c_void_p(buf.ctypes.data + o) for o in (0, 2, 4))

    def run(a=p, b=p, dtype=0, a_ld=3, b_ld=3, na=40, nb=1000, d=3, k=5, excl=0, r=p, q=p, dist=p, idx=p, cnt=p, ws=p, ws_bytes=MIB):
        return lib.d3p_pair_knn(None, a, b, dtype, a_ld, b_ld, na, nb, d, k, excl, r, q, dist, idx, cnt, ws, ws_bytes)
    assert lib.d3p_pair_knn_set_form(2) == 0
    need = lib.d3p_pair_knn_workspace(40, 1000, 3, 5)
    for name in ("a", "b", "q", "dist", "idx", "cnt"):
        assert run(**{name: None}) == -1 and b"null pointer" in lib.d3p_last_error(), name
    for name in ("a", "b", "r", "q", "dist", "idx", "cnt"):
        assert run(**{name: odd}) == -1 and b"not aligned to 4 bytes" in lib.d3p_last_error(), name
    assert run(ws=odd4) == -1 and b"not aligned to 8 bytes" in lib.d3p_last_error()
    for kw, said in (({"dtype": 2}, b"dtype must be 0 (float32) or 1 (int32)"), ({"na": 0}, b"na >= 1 and nb >= 1"), ({"nb": 0}, b"na >= 1 and nb >= 1"),
                     ({"d": 0, "a_ld": 0, "b_ld": 0}, b"d >= 1"), ({"a_ld": 2}, b"a_ld >= d"), ({"b_ld": -1}, b"b_ld >= d"),
                     ({"a_ld": 2 ** 62}, b"does not fit 63 bits"), ({"k": 0}, b"1 <= k <= 16"), ({"k": 17}, b"1 <= k <= 16"),
                     ({"excl": 2, "nb": 40}, b"exclude_diagonal must be 0 or 1"), ({"excl": 1}, b"na == nb is required")):
        assert run(**kw) == -1 and said in lib.d3p_last_error(), kw
    assert run(ws_bytes=need - 1) == -4 and run(ws=None) == -4 and b"workspace too small" in lib.d3p_last_error()
    for kw in ({"ws_bytes": need}, {"dtype": 1}, {"r": None, "cnt": None}, {"excl": 1, "nb": 40}, {"k": 16, "ws_bytes": 2 * 40 * 136}):
        assert run(**kw) == -1 and b"must be device memory" in lib.d3p_last_error(), kw                          # every value is fine
    assert lib.d3p_pair_knn_set_form(1) == 0
    assert run(ws=None, ws_bytes=0) == -1 and b"must be device memory" in lib.d3p_last_error()                   # the wide form needs none
    assert not buf.any()


def test_source_text_rules():
    """What d3p_pair_knn.hip shares with d3p_pair_stats.hip it takes from d3p_pair_tile.h (tests/test_fidelity_host.py holds every walker
    to that); what is its own stays: the guard of 4096 tiles ahead of the forced form, and k refused between the shape and the diagonal."""
    import re
    text = open(os.path.join(ROOT, "d3p_amd", "csrc", "d3p_pair_knn.hip")).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["d3p_device.h", "d3p_host.h", "d3p_pair_tile.h"]
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "sqrtf(" not in code and code.count("pair_sqrt(") == 1 and "__fmaf_rn(" not in code and "pair_chain(va[ki], vb[kj], q[ki][kj])" in code
    assert code.count("pair_admissible(i, j, a.nb, a.excl)") == 2 and code.count("pair_key(") == 2 and "pk_make" not in code
    assert not re.search(r"#define D3P_PK_(T|C|LD|WAVES|NONE|FORM_WIDE|FORM_SPLIT|WIDE_MIN_TILES)\b", text)
    assert code.index("pair_tiles(na) > D3P_PK_MAX_GROUPS) return D3P_PAIR_FORM_WIDE") < code.index("pair_form(g_pk_form, pair_tiles(na), pk_segments(na, nb))")
    assert code.index("pair_check_pair(") < code.index("1 <= k <= %d is required") < code.index("pair_check_diagonal(")
    assert 'pair_set_form("d3p_pair_knn_set_form", form, &g_pk_form)' in code and "pair_launch_merged(" in code


def test_python_layer_refuses_before_the_device(monkeypatch):
    import d3p_amd._lib as L
    from d3p_amd import neighbours as N
    monkeypatch.setattr(L, "require_device", lambda: pytest.fail("neighbours reached require_device"))
    a, b = torch.zeros((8, 3)), torch.zeros((5, 3))
    for fn in (lambda x, y: N.knn(x, y, 2), lambda x, y: N.ball_counts(x, y, torch.zeros(y.shape[0])), lambda x, y: N.prdc(x, y, 2)):
        with pytest.raises(ValueError, match="one dtype for both"):
            fn(a, b.to(torch.int32))
        with pytest.raises(ValueError, match="CUDA tensor"):              # every value is fine; the tensors are the host's
            fn(a, b)
    for k in (0, 17, 2.0, True):
        for fn in (lambda: N.knn(a, b, k), lambda: N.kth_neighbour(a, k), lambda: N.prdc(a, b, k)):
            with pytest.raises(ValueError, match=r"k must be an int in \[1, 16\]"):
                fn()
    with pytest.raises(ValueError, match="8 rows against 5"):
        N.knn(a, b, 1, exclude_diagonal=True)
    with pytest.raises(ValueError, match=r"synthetic: 5 rows; at least k \+ 1 = 6"):
        N.prdc(a, b, 5)
