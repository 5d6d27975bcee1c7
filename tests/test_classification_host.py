"""d3p_amd.classification (confusion counts per draw, ROC histogram, AUC, calibration), host side: the module and its C entries exist,
every refusal is raised before a device is touched, the bin map of d3p_binary_curve is order-preserving over the float32 patterns of
[0, 1], the certificate auc_lo <= AUC <= auc_hi holds against the exact Mann-Whitney value, the derived values are right on small
counts -- and the new translation unit shares the outcome rule, the link and the tile instead of copying them."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from . import classification_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "d3p_amd", "csrc")


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("classification reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


# ------------------------------------------------------------------------------- surface
def test_module_surface_and_lazy_import():
    import d3p_amd
    from d3p_amd import classification as CL
    assert d3p_amd.classification is CL and "classification" in d3p_amd.__all__
    assert CL.__all__ == ["predictive_confusion", "posterior_predictive_confusion", "binary_curve", "classification_report", "ConfusionCounts",
                          "BinaryCurve", "ClassificationReport"]
    assert CL.ConfusionCounts._fields == ("agree", "n_nan", "tp", "fp", "n_pos", "n_neg", "n_rows", "thresholds")
    assert CL.BinaryCurve._fields == ("hist", "calib", "n_pos", "n_neg", "pairs_concordant", "pairs_same_bin", "auc", "auc_lo", "auc_hi", "ks",
                                      "ece", "mce", "bins")
    assert CL.CURVE_BINS == R.BINS == 0x7E001 and CL.MAX_THRESHOLDS == 4 and CL.MAX_CURVE_ROWS == 2 ** 27
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.classification' not in sys.modules; " \
           "d3p_amd.classification; assert 'd3p_amd.classification' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_header_and_binding_declare_the_symbols():
    import d3p_amd._lib as L
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    assert re.search(r"#define D3P_CONF_THRESHOLDS 4\b", hdr) and re.search(r"#define D3P_CURVE_BINS 0x7E001\b", hdr)
    arity = {"d3p_predict_confusion": 15, "d3p_binary_curve": 10, "d3p_binary_curve_workspace": 0, "d3p_predict_confusion_set_strips": 1}
    for name, n in arity.items():
        args = re.search(r"\b" + name + r"\(([^)]*)\);", hdr).group(1)
        assert (0 if args.strip() == "void" else args.count(",") + 1) == n == len(L.SIGNATURES[name][1]), name
    assert os.path.join(CSRC, "d3p_classify.hip") in L._SRC and os.path.join(CSRC, "d3p_classify.hip") in L._DEPS
    lib = L.load()
    assert lib.d3p_abi_version() == 9
    for name in arity:
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.d3p_binary_curve_workspace() == 8 * 2 * ((R.BINS + 2047) // 2048)


def test_new_translation_unit_shares_the_rules_and_keeps_clear_of_the_pinned_headers():
    with open(os.path.join(CSRC, "d3p_classify.hip")) as f:
        text = f.read()
    includes = re.findall(r'#include\s+"([^"]+)"', text)
    assert sorted(includes) == ["d3p_device.h", "d3p_glm_tile.h", "d3p_host.h", "d3p_outcome.h"]
    assert "d3p_row_sums.h" not in text and "d3p_colreduce.h" not in text
    assert "glm_outcome<D3P_FAMILY_LOGREG>(" in text and "glm_mean<D3P_FAMILY_LOGREG>(" in text
    assert "stage_obs_keys<D3P_FAMILY_LOGREG>(" in text and "tile_product(" in text and "tile_scatter(" in text
    for own_rule in ("bernoulli_draw(", "sigmoid_probs(", "poisson_draw(", "normal_site_value(", "expf(", "1.0f / den", "loglik_value",
                     "bits_to_uniform(", "threefry2x32("):
        assert own_rule not in text, own_rule
    for pinned in ("cdiv(*tiles,", "? cdiv(*", "row_workspace_check(", ": the workspace must be", "hipFuncSetAttribute", "147456"):
        assert pinned not in text, pinned
    assert "extern __shared__" not in text                       # static LDS only


# ------------------------------------------------------------------------------- Python refusals, no device
def _logreg(d=3, intercept=True):
    from d3p_amd.models import LogisticRegression
    return LogisticRegression(d, intercept=intercept)


def test_models_and_guides_are_refused_before_the_device(no_device):
    from d3p_amd import classification as CL
    from d3p_amd.models import (AutoDiagonalNormal, GaussianMean, LinearRegression, MeanFieldGuide, PoissonRegression, VAEModel)
    X, y = np.zeros((6, 3), np.float32), np.zeros(6, np.float32)
    good = {"w": np.zeros((4, 3), np.float32), "intercept": np.zeros(4, np.float32)}
    k = torch.zeros(2, dtype=torch.int32)
    for bad in (GaussianMean(3), VAEModel(2, 4), LinearRegression(3), PoissonRegression(3)):
        with pytest.raises(TypeError, match="unsupported model"):
            CL.predictive_confusion(k, bad, good, X, y)
        with pytest.raises(TypeError, match="unsupported model"):
            CL.posterior_predictive_confusion(k, 4, bad, (X, y), None, {})
        with pytest.raises(TypeError, match="unsupported model"):
            CL.classification_report(k, 4, bad, (X, y), None, {})
    model = _logreg()
    for guide in (None, MeanFieldGuide(model), "auto"):
        with pytest.raises(TypeError, match="guide"):
            CL.posterior_predictive_confusion(k, 4, model, (X, y), guide, {})
        with pytest.raises(TypeError, match="guide"):
            CL.classification_report(k, 4, model, (X, y), guide, {})
    guide = AutoDiagonalNormal(model)
    params = {"auto_loc": np.zeros(4, np.float32), "auto_scale": np.ones(4, np.float32)}
    with pytest.raises(ValueError, match="n must be"):
        CL.posterior_predictive_confusion(k, 0, model, (X, y), guide, params)
    with pytest.raises(ValueError, match="params"):
        CL.posterior_predictive_confusion(k, 4, model, (X, y), guide, None)
    with pytest.raises(ValueError, match="y is missing"):
        CL.posterior_predictive_confusion(k, 4, model, (X,), guide, params)
    with pytest.raises(TypeError, match="rng_key"):                 # the last check before the device: a CPU key
        CL.posterior_predictive_confusion(k, 4, model, (X, y), guide, params)
    with pytest.raises(TypeError, match="rng_key"):
        CL.classification_report(k, 4, model, (X, y), guide, params)
    with pytest.raises(TypeError, match="rng_key"):
        CL.predictive_confusion(k, model, good, X, y)


def test_labels_thresholds_and_bins_are_refused_before_the_device(no_device):
    from d3p_amd import classification as CL
    from d3p_amd.models import AutoDiagonalNormal
    model = _logreg()
    X = np.zeros((6, 3), np.float32)
    good = {"w": np.zeros((4, 3), np.float32), "intercept": np.zeros(4, np.float32)}
    k = torch.zeros(2, dtype=torch.int32)
    for bad_y in (np.array([0, 1, 2, 0, 1, 0]), np.array([0, 1, -1, 0, 1, 0]), np.array([0, 1, 0.5, 0, 1, 0], np.float32),
                  np.array([0, 1, np.nan, 0, 1, 0], np.float32), torch.tensor([0, 1, 0, 3, 1, 0])):
        with pytest.raises(ValueError, match="y"):
            CL.predictive_confusion(k, model, good, X, bad_y)
        with pytest.raises(ValueError, match="y"):
            CL.posterior_predictive_confusion(k, 4, model, (X, bad_y), AutoDiagonalNormal(model),
                                              {"auto_loc": np.zeros(4, np.float32), "auto_scale": np.ones(4, np.float32)})
    with pytest.raises(ValueError, match="labels expected|y"):
        CL.predictive_confusion(k, model, good, X, np.zeros(5))
    y = np.array([0, 1, 1, 0, 1, 0])
    with pytest.raises(ValueError, match="at most 4"):
        CL.predictive_confusion(k, model, good, X, y, thresholds=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError, match="thresholds"):
        CL.predictive_confusion(k, model, good, X, y, thresholds=("a",))
    assert CL._thresholds(0.5) == (0.5,) and CL._thresholds(()) == () and np.isnan(CL._thresholds([float("nan"), 1])[0])
    assert CL._thresholds([0.1]) == (float(np.float32(0.1)),)                     # held as the float32 the kernel compares with
    params = {"auto_loc": np.zeros(4, np.float32), "auto_scale": np.ones(4, np.float32)}
    for bad_bins in (0, 65, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="bins"):
            CL.classification_report(k, 4, model, (X, y), AutoDiagonalNormal(model), params, bins=bad_bins)
        with pytest.raises(ValueError, match="bins"):
            CL.binary_curve(torch.zeros(6), y, bins=bad_bins)


def test_binary_curve_refusals_before_the_device(no_device):
    from d3p_amd import classification as CL
    y = np.array([0, 1, 1, 0])
    with pytest.raises(TypeError, match="CUDA tensor"):
        CL.binary_curve(np.zeros(4, np.float32), y)
    with pytest.raises(TypeError, match="CUDA tensor"):
        CL.binary_curve(torch.zeros(4), y)
    with pytest.raises(TypeError, match="float32"):
        CL.binary_curve(torch.zeros(4, dtype=torch.float64), y)
    with pytest.raises(ValueError, match="shape"):
        CL.binary_curve(torch.zeros(2, 2), y)
    with pytest.raises(ValueError, match="shape"):
        CL.binary_curve(torch.zeros(0), y)
    huge = torch.zeros(1).expand(2 ** 27 + 1)                       # (a view: no memory)
    with pytest.raises(ValueError, match=r"2\^27"):
        CL.binary_curve(huge, y)


# ------------------------------------------------------------------------------- C refusals, no device
def test_c_refusals_that_need_no_device_leave_the_outputs_alone():
    import d3p_amd._lib as L
    lib = L.load()
    buf = np.full(64, 0x5A5A5A5A5A5A5A5A, np.uint64)
    before = buf.copy()
    p = buf.ctypes.data
    tau = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    ok = L.LogregModel(3, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LOGREG, L.D3P_GUIDE_SOFTPLUS, 0.0)
    conf = lambda ms, X=p, y=p, rows=4, d=3, lat=p, ld=3, w_off=0, b_col=-1, n=1, keys=p, tau_=tau, T=1, out=p: \
        lib.d3p_predict_confusion(None, C.byref(ms) if ms is not None else None, X, y, rows, d, lat, ld, w_off, b_col, n, keys, tau_, T, out)
    assert conf(None) == -1 and b"null model" in lib.d3p_last_error()
    assert conf(ok, y=None) == -1 and b"null" in lib.d3p_last_error()
    for name in ("X", "lat", "keys", "out"):
        assert conf(ok, **{name: None}) == -1 and b"null" in lib.d3p_last_error(), name
    assert conf(ok, rows=0) == -1 and b"rows must be" in lib.d3p_last_error()
    assert conf(ok, d=4) == -1 and b"differs" in lib.d3p_last_error()
    assert conf(ok, n=0) == -1 and b"n must be" in lib.d3p_last_error()
    assert conf(ok, T=5) == -1 and b"thresholds" in lib.d3p_last_error()
    assert conf(ok, T=-1) == -1 and b"thresholds" in lib.d3p_last_error()
    assert conf(ok, tau_=None) == -1 and b"tau" in lib.d3p_last_error()
    assert conf(ok, ld=2) == -1 and conf(ok, b_col=0) == -1 and conf(ok, rows=2 ** 32) == -1
    assert conf(ok) == -1 and b"device memory" in lib.d3p_last_error()            # host pointers never reach a kernel
    for fam in (L.D3P_FAMILY_LINREG, L.D3P_FAMILY_POISSON, L.D3P_FAMILY_GAUSS_MEAN):
        other = L.LogregModel(3, 0, 1.0, 1.0, 1.0, 1.0, fam, L.D3P_GUIDE_SOFTPLUS, 1.0)
        assert conf(other) == -3 and b"logistic regression only" in lib.d3p_last_error()
    sites = L.LogregModel(3, 1, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LOGREG, L.D3P_GUIDE_EXP_SITES, 0.0)
    assert conf(sites, b_col=3, ld=4) == -3 and b"D3P_GUIDE_EXP_SITES" in lib.d3p_last_error()
    assert lib.d3p_predict_confusion_set_strips(-1) == -1 and lib.d3p_predict_confusion_set_strips(65536) == -1
    assert lib.d3p_predict_confusion_set_strips(7) == 0 and lib.d3p_predict_confusion_set_strips(0) == 0

    nb = lib.d3p_binary_curve_workspace()
    curve = lambda p_=p, y=p, rows=4, B=10, hist=p, calib=p, summary=p, ws=p, nbytes=nb: \
        lib.d3p_binary_curve(None, p_, y, rows, B, hist, calib, summary, ws, nbytes)
    for name in ("p_", "y", "hist", "calib", "summary", "ws"):
        assert curve(**{name: None}) == -1 and b"null" in lib.d3p_last_error(), name
    assert curve(rows=0) == -1 and b"rows must be" in lib.d3p_last_error()
    assert curve(rows=2 ** 27 + 1) == -1 and b"2^27" in lib.d3p_last_error()
    assert curve(B=0) == -1 and curve(B=65) == -1 and b"reliability bins" in lib.d3p_last_error()
    for name in ("p_", "y", "hist"):
        assert curve(**{name: p + 2}) == -1 and b"aligned to 4" in lib.d3p_last_error(), name
    for name in ("calib", "summary", "ws"):
        assert curve(**{name: p + 4}) == -1 and b"aligned to 8" in lib.d3p_last_error(), name
    assert curve(nbytes=nb - 1) == -1 and str(nb).encode() + b" needed" in lib.d3p_last_error()
    assert curve() == -1 and b"device memory" in lib.d3p_last_error()
    assert np.array_equal(buf, before)


# ------------------------------------------------------------------------------- the bin map
def _patterns():
    """Every float32 bit pattern of [0, 1] at stride 7, plus the edges."""
    bits = np.arange(0, 0x3F800000 + 1, 7, dtype=np.uint32)
    edges = np.array([0, 1, 0x3EFFFFFF, 0x3F000000, 0x3F000001, 0x3F7FFFFF, 0x3F800000], np.uint32)
    return np.unique(np.concatenate([bits, edges])).view(np.float32)


def test_bin_map_is_non_decreasing_over_the_patterns_of_the_unit_interval():
    p = _patterns()                                                   # ascending patterns = ascending values
    assert p[0] == 0.0 and p[-1] == 1.0 and np.all(np.diff(p) > 0)
    b = R.bin_of(p)
    assert np.all(np.diff(b) >= 0) and b.min() == 0 and b.max() == 0x7E000 == R.BINS - 1
    assert b[0] == 0 and b[-1] == 0x7E000
    edge = lambda bits: int(R.bin_of(np.array([bits], np.uint32).view(np.float32))[0])
    assert edge(0x3EFFFFFF) == 0x3EFFF and edge(0x3F000000) == 0x3F000 and edge(0x3F000001) == 0x3F001   # 1 - p = 0x3EFFFFFE
    assert edge(0x3F7FFFFF) == 0x7E000 - (0x33800000 >> 12) and edge(0x3F800000) == 0x7E000     # 1 - p = 2^-24 there
    assert int(R.bin_of(np.array([-0.0], np.float32))[0]) == 0
    # strictly order-preserving ACROSS bins: two scores in different bins are ordered as their bins are (that is: non-decreasing)
    hi = p[p >= np.float32(0.5)]
    mirror = np.float32(1.0) - hi                                      # float32 arithmetic
    assert mirror.dtype == np.float32 and np.array_equal(mirror.astype(np.float64), 1.0 - hi.astype(np.float64))   # 1 - p is exact


def test_exact_auc_lies_inside_the_certificate_on_random_scores():
    rng = np.random.default_rng(11)
    for rows, scale in ((1, 1.0), (2, 1.0), (500, 1.0), (5000, 3.0), (20000, 8.0), (20000, 0.05)):
        t = rng.normal(size=rows) * scale
        p = (1.0 / (1.0 + np.exp(-t))).astype(np.float32)
        y = (rng.random(size=rows) < p).astype(np.int64)
        hist, calib, summary = R.curve(p, y, 10)
        lo, mid, hi = R.auc_bounds(summary)
        exact = R.exact_auc(p, y)
        if np.isnan(exact):
            assert summary[1] * summary[2] == 0 and np.isnan(mid)
            continue
        assert lo <= exact <= hi and lo <= mid <= hi, (rows, scale, lo, exact, hi)
        assert hist.sum() == rows and calib[0].sum() == rows and calib[1].sum() == y.sum() == summary[1]
        assert summary[5] / (float(summary[1]) * float(summary[2])) == R.ks_statistic(hist, summary[1], summary[2])   # bottom up = top down
        assert abs(mid - exact) <= (hi - lo) / 2 + 1e-15
    # scores that pile up in few values: the certificate widens, and still holds
    p = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32), size=3000)
    y = (rng.random(size=3000) < p).astype(np.int64)
    lo, mid, hi = R.auc_bounds(R.curve(p, y, 4)[2])
    assert lo < R.exact_auc(p, y) < hi and hi - lo > 0.01 and abs(mid - R.exact_auc(p, y)) < 1e-12   # (ties at half weight: auc IS exact here)


def test_auc_is_exact_when_each_bin_holds_one_value():
    """1000 multiples of 2^-10 in [0, 1): 10 significant bits, fewer than the 11 the map keeps at either end, so no two share a bin."""
    rng = np.random.default_rng(3)
    grid = (np.arange(1000) / 1024.0).astype(np.float32)
    assert np.unique(R.bin_of(grid)).size == 1000
    p = rng.choice(grid, size=20000)
    y = (rng.random(size=20000) < p).astype(np.int64)
    summary = R.curve(p, y, 16)[2]
    lo, mid, hi = R.auc_bounds(summary)
    exact = R.exact_auc(p, y)
    assert summary[4] > 0 and lo < exact < hi                         # ties exist (equal scores), each at half weight
    assert abs(mid - exact) <= 4 * np.finfo(np.float64).eps * exact   # the same rational number, rounded along two routes
    # all scores distinct: no pair shares a bin, and the three coincide
    q = rng.permutation(grid)
    yq = (rng.random(size=1000) < q).astype(np.int64)
    s = R.curve(q, yq, 16)[2]
    assert s[4] == 0 and R.auc_bounds(s)[0] == R.auc_bounds(s)[2]
    assert abs(R.auc_bounds(s)[1] - R.exact_auc(q, yq)) <= 4 * np.finfo(np.float64).eps


def test_invalid_scores_and_labels_are_counted_and_left_out():
    p = np.array([0.25, np.nan, -0.5, 1.5, 0.75, 0.5, -0.0, 1.0], np.float32)
    y = np.array([0, 1, 1, 0, 1, 2, 1, 0])
    hist, calib, summary = R.curve(p, y, 4)
    assert summary[0] == 4 and hist.sum() == 4 and calib[0].tolist() == [1, 1, 0, 2] and calib[1].tolist() == [1, 0, 0, 1]
    assert calib[2].tolist() == [0, int(0.25 * 2 ** 36), 0, int(0.75 * 2 ** 36) + 2 ** 36]   # 0.25 x 4 = 1.0: the second bin
    assert summary[1:5] == [2, 2, 1, 0]                               # the positives 0.75 > 0.25; -0.0 is below both negatives


# ------------------------------------------------------------------------------- the derived values
def test_confusion_counts_derive_in_float64_one_operation_per_step():
    from d3p_amd import classification as CL
    tp = np.array([[30, 10], [0, 0], [40, 40]], np.int64)
    fp = np.array([[5, 0], [0, 0], [60, 60]], np.int64)
    agree = np.array([70, 50, 40], np.int64)
    for wrap in (lambda a: a, lambda a: torch.tensor(a)):
        c = CL.ConfusionCounts(wrap(agree), wrap(np.zeros(3, np.int64)), wrap(tp), wrap(fp), 40, 60, 100, (0.5, 0.9))
        val = lambda x: np.asarray(x, np.float64)
        f = np.float64
        with np.errstate(all="ignore"):
            assert np.array_equal(val(c.sampled_accuracy), agree / f(100))
            assert np.array_equal(val(c.fn), 40 - tp) and np.array_equal(val(c.tn), 60 - fp)
            assert np.array_equal(val(c.accuracy), (tp + (60 - fp)) / f(100))
            assert np.array_equal(val(c.tpr), tp / f(40)) and np.array_equal(val(c.fpr), fp / f(60))
            assert np.array_equal(val(c.precision), tp.astype(f) / (tp + fp).astype(f), equal_nan=True)
            assert np.isnan(val(c.precision)[1]).all()                   # 0 / 0: NaN, not clamped
            assert np.array_equal(val(c.f1), (2 * tp).astype(f) / (2 * tp + fp + (40 - tp)).astype(f))
            assert np.array_equal(val(c.balanced_accuracy), (tp / f(40) + (60 - fp) / f(60)) / 2.0)
    none = CL.ConfusionCounts(agree, agree * 0, tp, fp, 0, 100, 100, (0.5, 0.9))
    with np.errstate(all="ignore"):
        assert np.isnan(none.tpr[1]).all() and np.isinf(none.tpr[0]).all()   # no positives: 0 / 0 and x / 0 as IEEE has them


def test_calibration_errors_follow_the_restatement():
    from d3p_amd import classification as CL
    rng = np.random.default_rng(4)
    p = rng.random(size=4000).astype(np.float32)
    y = (rng.random(size=4000) < p ** 2).astype(np.int64)             # miscalibrated on purpose
    _, calib, _ = R.curve(p, y, 10)
    ece, mce = CL._calibration_errors(calib, 4000)
    assert (ece, mce) == R.calibration_errors(calib, 4000)
    assert 0.1 < ece < 0.25 and ece <= mce                             # E|p - p^2| = 1/2 - 1/3 = 1/6 for uniform scores
