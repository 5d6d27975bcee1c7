"""CRPS and PIT calibration (d3p_amd.scoring, d3p_col_crps), host side: the three restatements of the rule in tests/scoring_ref.py against
each other within the derived bound, the Brier identity, n = 1, the PIT histogram by hand, the declared symbols, and every argument check
of the module and of the C entry that needs no device."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import scoring_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_N = (1, 2, 3, 9, 31)


def _cases():
    return [(f"{kind} n={n}", kind, n) for kind in SR.KINDS for n in HOST_N]


def _as_float(exact):
    return np.array([[np.nan if v is None else float(v) for v in row] for row in exact], np.float64)


@pytest.mark.parametrize("name,kind,n", _cases(), ids=[c[0] for c in _cases()])
def test_the_three_restatements_agree_within_the_bound(name, kind, n):
    m = SR.matrix(kind, n, 9)
    for r in range(len(SR.y_kinds(m))):
        y = SR.observations(m, SR.rotation(m, r))
        exact = _as_float(SR.score_exact(m, y))
        tol = SR.bound(m, y, exact)
        at, at_counts = SR.score_at(m, y)
        pw, pw_counts = SR.score_pairwise(m, y)
        assert np.array_equal(at_counts, pw_counts)
        for what, got in (("score_at", at), ("score_pairwise", pw)):
            ok, worst = SR.within(got, exact, tol)
            assert ok, f"{name} rotation {r}: {what} misses the exact value by {worst} bounds"
        bad = SR.nonfinite(m, y)
        assert np.array_equal(np.isnan(exact[0]), bad) and np.array_equal(np.isnan(exact[2]), bad)
        assert np.array_equal(np.isnan(exact[1]), bad | (n == 1))


def test_the_counts_follow_ieee_comparison():
    m = np.array([[-0.0, 1.0, np.nan], [0.0, 2.0, 1.0], [1.0, np.nan, 2.0], [-1.0, np.inf, 3.0]], np.float32)
    below, equal = SR.counts(m, np.array([0.0, np.inf, np.nan], np.float32))
    assert below.tolist() == [1, 2, 0] and equal.tolist() == [2, 1, 0]
    below, equal = SR.counts(m, np.array([-0.0, 2.0, 2.0], np.float32))
    assert below.tolist() == [1, 1, 1] and equal.tolist() == [2, 1, 1]
    assert SR.nonfinite(m, np.zeros(3, np.float32)).tolist() == [False, True, True]
    assert SR.nonfinite(m, np.array([np.inf, 0.0, 0.0], np.float32)).tolist() == [True, True, True]


@pytest.mark.parametrize("n", [1, 2, 10, 31, 257])
def test_binary_draws_score_the_brier_score_of_their_frequency(n):
    m = SR.matrix("binary", n, 22)
    for yv in (0, 1):
        y = np.full(22, yv, np.int32)
        exact = SR.score_exact(m, y)
        p = [Fraction(int(m[:, c].sum()), n) for c in range(22)]
        assert [exact[0][c] for c in range(22)] == [(p[c] - yv) ** 2 for c in range(22)]          # exactly, as rationals
        at, counts = SR.score_at(m, y)
        want = np.array([float((p[c] - yv) ** 2) for c in range(22)])
        assert np.all(np.abs(at[0] - want) <= SR.bound(m, y)[0])
        assert np.array_equal(counts[1], (m == yv).sum(0)) and np.array_equal(counts[0], (m < yv).sum(0))
    assert set(np.unique(SR.matrix("binary", 257, 22))) == {0, 1}


def test_one_draw_scores_its_distance_and_has_no_fair_form():
    m = np.array([[1.5, -2.0, 7.0]], np.float32)
    y = np.array([0.25, -2.0, 9.0], np.float32)
    at, counts = SR.score_at(m, y)
    assert np.array_equal(at[0], [1.25, 0.0, 2.0]) and np.array_equal(at[2], at[0]) and np.array_equal(at[3], [0.0, 0.0, 0.0])
    assert np.isnan(at[1]).all()
    assert counts.tolist() == [[0, 0, 1], [0, 1, 0]]
    assert all(v is None for v in SR.score_exact(m, y)[1])


def test_fixed_columns_by_hand():
    # draws (1, 2, 4) against 3: A = 2 + 1 + 1 = 4, G = -2 (1 - 3) + 0 + 2 (4 - 3) = 6: mae 4/3, spread 6/9, crps 2/3, fair 4/3 - 1 = 1/3
    m = np.array([[4], [1], [2]], np.int32)
    y = np.array([3], np.int32)
    exact = SR.score_exact(m, y)
    assert [exact[r][0] for r in range(4)] == [Fraction(2, 3), Fraction(1, 3), Fraction(4, 3), Fraction(2, 3)]
    pw, counts = SR.score_pairwise(m, y)
    assert np.allclose(pw[:, 0], [2 / 3, 1 / 3, 4 / 3, 2 / 3], rtol=1e-15) and counts[:, 0].tolist() == [2, 0]


# ---------------------------------------------------------------- the PIT histogram
def test_pit_histogram_places_points_and_intervals_by_hand():
    from d3p_amd import scoring as SC
    lower = torch.tensor([0.0, 0.25, 1.0, 0.0, 0.05, 0.3, 0.999])
    upper = torch.tensor([0.0, 0.25, 1.0, 1.0, 0.25, 0.3, 0.999])
    h = SC.pit_histogram(lower, upper, bins=10)
    assert h.shape == (10,) and h.dtype == torch.float64
    # points: 0 -> bin 0, 0.25 -> bin 2, 1.0 -> the last bin, 0.3 (float32: just above 0.3) -> bin 3, 0.999 -> bin 9
    # intervals: [0, 1] gives 0.1 to every bin; [0.05, 0.25] gives 0.25, 0.5, 0.25 to bins 0, 1, 2
    want = torch.tensor([1.35, 0.6, 1.35, 1.1, 0.1, 0.1, 0.1, 0.1, 0.1, 2.1], dtype=torch.float64)
    assert torch.allclose(h, want, atol=1e-6), h
    assert abs(float(h.sum()) - 7.0) < 1e-12
    h4 = SC.pit_histogram(torch.tensor([0.5, 0.0]), torch.tensor([0.5, 0.5]), bins=4)
    assert torch.equal(h4, torch.tensor([0.5, 0.5, 1.0, 0.0], dtype=torch.float64))
    assert SC.pit_histogram(torch.zeros(0), torch.zeros(0), bins=3).tolist() == [0.0, 0.0, 0.0]
    rng = np.random.default_rng(3)
    lo = np.sort(rng.integers(0, 101, size=(2, 500)), axis=0) / 100.0
    h = SC.pit_histogram(torch.tensor(lo[0], dtype=torch.float32), torch.tensor(lo[1], dtype=torch.float32), bins=7)
    assert abs(float(h.sum()) - 500.0) < 1e-9 and bool((h >= 0).all())


def test_pit_histogram_refuses_bad_arguments():
    from d3p_amd import scoring as SC
    a = torch.tensor([0.1, 0.2])
    for bins in (0, -1, 2.5, None, True, "10"):
        with pytest.raises(ValueError, match="bins"):
            SC.pit_histogram(a, a, bins=bins)
    for lo, hi in ((a, a[:1]), (a.reshape(1, 2), a.reshape(1, 2)), ([0.1], [0.2])):
        with pytest.raises(ValueError, match="1-D tensors"):
            SC.pit_histogram(lo, hi)
    for lo, hi in ((a, a - 0.05), (a - 0.5, a), (a, a + 1.0), (torch.tensor([float("nan")]), torch.tensor([0.5]))):
        with pytest.raises(ValueError, match="0 <= lower <= upper <= 1"):
            SC.pit_histogram(lo, hi)


# ---------------------------------------------------------------- the declared surface
def test_symbols_are_declared_and_exported():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import scoring as SC
    hdr = open(os.path.join(ROOT, "include", "d3p_hip.h")).read()
    assert re.search(r"\bint d3p_col_crps\(void\* stream, const void\* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t cols,\s+"
                     r"const void\* y_dev,[^\n]*\n\s+float\* out_dev, int64_t out_ld,[^\n]*\n\s+uint32_t\* counts_dev, int64_t counts_ld[^\n]*\);", hdr)
    assert re.search(r"\buint32_t d3p_col_crps_max_n\(void\);", hdr) and re.search(r"\buint32_t d3p_col_crps_cols_per_group\(uint32_t n\);", hdr)
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    assert len(L.SIGNATURES["d3p_col_crps"][1]) == 11 and L.SIGNATURES["d3p_col_crps_max_n"][1] == []
    assert any(p.endswith("d3p_crps.hip") for p in L._SRC) and all(any(p.endswith(h) for p in L._DEPS) for h in ("d3p_colsort.h", "d3p_crps.h", "d3p_crps_kernel.h"))
    lib = L.load()
    most = lib.d3p_col_crps_max_n()
    assert most == lib.d3p_col_hpdi_max_n() == SC.draws_limit() == 144 * 1024 // 8
    for n in (0, 1, 2, 1152, 1153, 4608, 4609, most, most + 1, 2 ** 32 - 1):       # the forms and their limits are k_col_hpdi's
        assert lib.d3p_col_crps_cols_per_group(n) == lib.d3p_col_hpdi_cols_per_group(n)
    assert d3p_amd.scoring is SC and "scoring" in d3p_amd.__all__
    assert SC.CRPSResult._fields == ("crps", "se", "mae", "spread", "pit_histogram", "n_draws", "n_rows", "pointwise")
    for name in ("score_draws", "crps", "pit", "pit_histogram", "draws_limit", "predictive_crps", "posterior_predictive_crps", "compare_scores"):
        assert name in SC.__all__ and callable(getattr(SC, name))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"`d3p_col_crps`[^\n]*crps_ensemble", integration)
    sort = open(os.path.join(ROOT, "d3p_amd", "csrc", "d3p_colsort.h")).read()
    texts = {src: open(os.path.join(ROOT, "d3p_amd", "csrc", src)).read() for src in ("d3p_hpdi.hip", "d3p_crps_kernel.h", "d3p_crps.hip")}
    assert sort.count("void h_step") == 1 and all("void h_step" not in text for text in texts.values())      # one network, defined once
    # the kernel is compiled in the HPDI translation unit, behind the keys and the sort; the entry's file includes neither
    assert '#include "d3p_colsort.h"' in texts["d3p_hpdi.hip"] and '#include "d3p_crps_kernel.h"' in texts["d3p_hpdi.hip"]
    assert "h_sort<COLS>" in texts["d3p_crps_kernel.h"] and "h_stage<COLS>" in texts["d3p_crps_kernel.h"]
    assert "#include" not in sort and "col_crps_launch" in texts["d3p_crps.hip"]


def test_the_c_entry_refuses_on_the_host_as_declared():
    """Everything d3p_col_crps checks before it asks whether a pointer is device memory, in the order of d3p_col_hpdi: the buffers here
    are host memory and are never reached."""
    import d3p_amd._lib as L
    lib = L.load()
    most = lib.d3p_col_crps_max_n()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)

    def run(m=p, dtype=0, ld=8, n=4, cols=8, y=p, out=p, out_ld=8, counts=p, counts_ld=8):
        return lib.d3p_col_crps(None, m, dtype, ld, n, cols, y, out, out_ld, counts, counts_ld)
    for kw in ({"m": None}, {"y": None}, {"out": None}, {"counts": None}):
        assert run(**kw) == -1 and b"null" in lib.d3p_last_error()
    for name in ("m", "y", "out", "counts"):
        assert run(**{name: C.c_void_p(buf.ctypes.data + 2)}) == -1 and b"aligned" in lib.d3p_last_error()
    assert run(dtype=2) == -1 and run(dtype=-1) == -1 and b"dtype" in lib.d3p_last_error()
    assert run(n=0) == -1 and b"n >= 1" in lib.d3p_last_error()
    assert run(ld=7) == -1 and b"ld >= cols" in lib.d3p_last_error()
    assert run(out_ld=7) == -1 and b"out_ld" in lib.d3p_last_error()
    assert run(counts_ld=7) == -1 and b"counts_ld" in lib.d3p_last_error()
    assert run(ld=-1) == -1 and run(out_ld=-1) == -1 and run(counts_ld=-1) == -1
    assert run(n=most + 1) == -3 and str(most).encode() in lib.d3p_last_error() and b"no streamed form" in lib.d3p_last_error()
    assert run(n=most + 1, cols=0, ld=0, out_ld=0, counts_ld=0) == -3 and run(n=2 ** 32 - 1) == -3
    assert run(n=0, cols=0) == -1                                                   # n is checked before cols == 0 returns
    assert run(cols=0) == 0 and run(cols=0, n=most) == 0                            # D3P_OK before any device question
    assert not buf.any()


# ---------------------------------------------------------------- host-side argument checks of the Python layer (no device)
def _models():
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    return LinearRegression(4, obs_scale=0.5), PoissonRegression(4), LogisticRegression(4)


def _args(n=10, rows=20, d=4):
    return {"w": np.zeros((n, d), np.float32)}, np.zeros((rows, d), np.float32), np.zeros(rows, np.float32)


def _guide(model):
    from d3p_amd.models import AutoDiagonalNormal
    return AutoDiagonalNormal(model)


def _calls(SC, model, s, X, y, n, **kw):
    return (lambda: SC.predictive_crps(None, model, s, X, y, **kw),
            lambda: SC.posterior_predictive_crps(None, n, model, (X, y), _guide(model), {}, **kw))


def test_the_model_free_functions_refuse_what_is_not_a_device_matrix():
    from d3p_amd import scoring as SC
    y = torch.zeros(2)
    for bad in (np.zeros((3, 2), np.float32), torch.zeros((3, 2)), torch.zeros((3,)), torch.zeros((3, 2), dtype=torch.float64)):
        for call in (lambda: SC.score_draws(bad, y), lambda: SC.crps(bad, y), lambda: SC.crps(bad, y, fair=True), lambda: SC.pit(bad, y)):
            with pytest.raises(ValueError, match="CUDA tensor"):
                call()


def test_observations_are_checked_against_the_matrix_dtype():
    from d3p_amd import scoring as SC
    f32, i32 = torch.float32, torch.int32
    assert SC._observations([1.0, 2.0], f32, 2, "t").dtype == f32 and SC._observations(np.array([1, 2]), f32, 2, "t").dtype == f32
    got = SC._observations(np.array([3.0, -0.0, 2147483647.0, -2147483648.0]), i32, 4, "t")
    assert got.dtype == i32 and got.tolist() == [3, 0, 2147483647, -2147483648]
    assert SC._observations(torch.tensor([5, 6], dtype=torch.int64), i32, 2, "t").tolist() == [5, 6]
    assert SC._observations(torch.tensor([[1.0], [2.0]]), f32, 2, "t").shape == (2,)
    for y, msg in (([1.0, 2.0, 3.0], "2 observations expected"), ([0.5, 1.0], "non-integral"), ([float("nan"), 1.0], "non-integral"),
                   ([float("inf"), 1.0], "int32's range"), ([2147483648.0, 0.0], "int32's range"),
                   (torch.tensor([2 ** 31, 0], dtype=torch.int64), "int32's range"), (torch.tensor([True, False]), "must hold"),
                   (torch.tensor([1j, 0j]), "must hold")):
        with pytest.raises(ValueError, match=msg):
            SC._observations(y, i32, 2, "t")
    with pytest.raises(ValueError, match="must hold"):
        SC._observations(torch.tensor([True, False]), f32, 2, "t")
    with pytest.raises(ValueError, match="not an array of numbers|must hold"):
        SC._observations(["a", "b"], f32, 2, "t")


def test_unsupported_models_and_guides_are_refused():
    from d3p_amd import scoring as SC
    from d3p_amd.models import GaussianMixtureModel
    lin, _, log = _models()
    s, X, y = _args()
    for model in (GaussianMixtureModel(), object()):
        for call in (lambda: SC.predictive_crps(None, model, s, X, y), lambda: SC.posterior_predictive_crps(None, 5, model, (X, y), None, {})):
            with pytest.raises(TypeError, match="unsupported model"):
                call()
    with pytest.raises(TypeError, match="guide"):
        SC.posterior_predictive_crps(None, 5, lin, (X, y), None, {})
    with pytest.raises(ValueError, match="n must be >= 1"):
        SC.posterior_predictive_crps(None, 0, lin, (X, y), _guide(lin), {})
    with pytest.raises(TypeError, match="rng_key"):                  # logistic outcomes ARE scored: the next check is the key's
        SC.predictive_crps(None, log, s, X, y)


def test_the_labels_are_read_and_checked():
    from d3p_amd import scoring as SC
    lin, poi, log = _models()
    s, X, y = _args()
    for model in (lin, poi, log):
        for call in (lambda: SC.predictive_crps(None, model, s, X), lambda: SC.posterior_predictive_crps(None, 5, model, (X,), _guide(model), {})):
            with pytest.raises(ValueError, match="y is missing"):
                call()
        for call in _calls(SC, model, s, X, y[:19], 5):
            with pytest.raises(ValueError, match="20 labels expected"):
                call()
    for bad, msg in ((np.full(20, -1.0, np.float32), "integers >= 0"), (np.full(20, 0.5, np.float32), "non-integral")):
        for call in _calls(SC, poi, s, X, bad, 5):
            with pytest.raises(ValueError, match=msg):
                call()
    for call in _calls(SC, log, s, X, np.full(20, 0.5, np.float32), 5):
        with pytest.raises(ValueError, match="non-integral"):
            call()
    given, drawn = _calls(SC, lin, s, X, np.full(20, 0.5), 5)        # float64 labels of a linear model are cast: the next check is met
    with pytest.raises(TypeError, match="rng_key"):
        given()
    with pytest.raises(ValueError, match="'auto_loc' is missing"):
        drawn()


def test_draw_limit_slab_and_bins_are_checked_before_the_key():
    from d3p_amd import scoring as SC
    lin, poi, _ = _models()
    most = SC.draws_limit()
    s, X, y = _args(n=most + 1, rows=3)
    for model in (lin, poi):
        for call in _calls(SC, model, s, X, y, most + 1, slab_bytes=1 << 40):
            with pytest.raises(ValueError, match=rf"n <= {most}\b"):
                call()
    s, X, y = _args()
    for model in (lin, poi):
        for call in _calls(SC, model, s, X, y, 10, slab_bytes=799):
            with pytest.raises(ValueError, match=r"written whole .* slab_bytes >= 800\b"):
                call()
        for slab_bytes in (0, -1, 1.5, None, True):
            for call in _calls(SC, model, s, X, y, 10, slab_bytes=slab_bytes):
                with pytest.raises(ValueError, match="slab_bytes"):
                    call()
        for bins in (0, 2.5, None, True):
            for call in _calls(SC, model, s, X, y, 10, bins=bins):
                with pytest.raises(ValueError, match="bins"):
                    call()
        with pytest.raises(TypeError, match="rng_key"):
            SC.predictive_crps(None, model, s, X, y, slab_bytes=800)


def test_compare_scores_refuses_what_it_cannot_pair():
    from d3p_amd import scoring as SC
    z = torch.zeros((), dtype=torch.float64)
    pw = {"crps": torch.tensor([1.0, 2.0, 4.0])}
    a = SC.CRPSResult(z, z, z, z, torch.zeros(10, dtype=torch.float64), 5, 3, pw)
    b = SC.CRPSResult(z, z, z, z, torch.zeros(10, dtype=torch.float64), 5, 3, {"crps": torch.tensor([2.0, 2.0, 2.0])})
    for x, y in ((a, a._replace(pointwise=None)), (a._replace(pointwise=None), a), (a, object()), ((1, 2), a)):
        with pytest.raises(ValueError, match="pointwise"):
            SC.compare_scores(x, y)
    with pytest.raises(ValueError, match="same rows"):
        SC.compare_scores(a, b._replace(n_rows=4))
    same = SC.compare_scores(a, a)
    assert float(same.crps_diff) == 0.0 and float(same.se_diff) == 0.0
    d = SC.compare_scores(a, b)                                      # differences (-1, 0, 2): mean 1/3, variance 7/3, se sqrt(7/9)
    assert abs(float(d.crps_diff) - 1.0 / 3.0) < 1e-15 and abs(float(d.se_diff) - (7.0 / 9.0) ** 0.5) < 1e-15
    assert float(SC.compare_scores(b, a).crps_diff) == -float(d.crps_diff)


def test_the_examples_take_the_crps_flag():
    for name in ("linear_regression", "poisson_regression"):
        src = open(os.path.join(ROOT, "examples", name + ".py")).read()
        assert "--crps" in src and "predictive_crps" in src
