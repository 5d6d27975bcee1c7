"""d3p_amd.classification on the GPU.  d3p_predict_confusion against the matrices the sibling entries store for the same latents and
keys -- mu from d3p_predict_mean_rows, v from d3p_predict_logreg -- at every edge of the tiling; d3p_binary_curve against the numpy
restatement (tests/classification_ref.py); the Python layer against the *_samples calls and the example's estimate_accuracy.
Everything the entries compute is an integer: every comparison is BY VALUE."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from d3p_amd import _lib as L
from d3p_amd import classification as CL
from d3p_amd import prediction as PR
from d3p_amd import predictive as Ps
from d3p_amd.models import AutoDiagonalNormal, DiagonalNormalGuide, LogisticRegression

from . import classification_ref as R
from .predictive_ref import key, logreg_params, np_

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _model_struct(d, intercept):
    return L.LogregModel(d, int(intercept), 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LOGREG, L.D3P_GUIDE_SOFTPLUS, 0.0)


def _problem(d, rows, n, intercept, seed):
    """X, the latent buffer (n, ld) with a padded ld, the weights at w_off and the intercept at b_col, random obs keys, 0 / 1 labels.
    The predictors have a spread of about 2: probabilities from 0.01 to 0.99."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, size=(rows, d)).astype(np.float32)
    ld, w_off, b_col = d + 3, 2, (0 if intercept else -1)
    lat = rng.normal(size=(n, ld)).astype(np.float32)
    lat[:, w_off:w_off + d] *= np.float32(4.0 / np.sqrt(d))
    if intercept:
        lat[:, b_col] = rng.uniform(-1, 2, size=n).astype(np.float32)
    keys = rng.integers(0, 2 ** 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
    y = (rng.random(size=rows) < 0.4).astype(np.float32)
    return X, lat, ld, w_off, b_col, keys, y


def _stored(Xd, latd, ld, w_off, b_col, kd, d, rows, n, intercept):
    """(mu, v) as numpy: what d3p_predict_mean_rows and d3p_predict_logreg store for these arguments."""
    lib = L.load()
    ms = _model_struct(d, intercept)
    mu = torch.empty((n, rows), dtype=torch.float32, device=DEV)
    L.check(lib.d3p_predict_mean_rows(L.stream_ptr(), C.byref(ms), L.ptr(Xd), rows, L.ptr(latd), ld, w_off, b_col, n, L.ptr(mu), rows))
    obs = torch.empty((n, rows), dtype=torch.int32, device=DEV)
    L.check(lib.d3p_predict_logreg(L.stream_ptr(), L.ptr(Xd), rows, d, L.ptr(latd), ld, w_off, b_col, n, L.ptr(kd), L.ptr(obs)))
    return np_(mu), np_(obs)


def _fused(Xd, yd, latd, ld, w_off, b_col, kd, d, rows, n, intercept, tau):
    """d3p_predict_confusion into an out that held 0xFF bytes: (10, n) int64 as numpy."""
    out = torch.full((10, n), -1, dtype=torch.int64, device=DEV)          # every byte 0xFF: the entry zeroes what it adds into
    ms = _model_struct(d, intercept)
    taus = (C.c_float * 4)(*tau) if tau else None
    L.check(L.load().d3p_predict_confusion(L.stream_ptr(), C.byref(ms), L.ptr(Xd), L.ptr(yd), rows, d, L.ptr(latd), ld, w_off, b_col, n, L.ptr(kd),
                                           taus, len(tau), L.ptr(out)))
    return np_(out)


def _thresholds(T, mu):
    """T thresholds: a value some stored mu equals exactly (so that >= and > differ), then 0, 1 and NaN."""
    hit = float(mu[mu.shape[0] // 2, mu.shape[1] // 2])
    return [hit, 0.0, 1.0, NAN][:T]


# ------------------------------------------------------------------------------- the C entry against the stored matrices
ROWS = [1, 31, 32, 33, 127, 128, 129, 389]
DRAWS = [1, 31, 33, 128, 129]
DIMS = [1, 4, 33]


@pytest.mark.parametrize("rows", ROWS)
def test_c_entry_equals_the_counts_of_the_stored_matrices(gpu, rows):
    """Every rows value with every n; d, the intercept and T cycle so that each value meets each rows value's neighbours: over the 40
    cases every (d, intercept, T) combination occurs."""
    i = ROWS.index(rows)
    for j, n in enumerate(DRAWS):
        d, intercept, T = DIMS[(i + j) % 3], bool((i + j // 3) % 2), (0, 1, 4)[(i + 2 * j) % 3]
        X, lat, ld, w_off, b_col, keys, y = _problem(d, rows, n, intercept, 31 * d + 7 * rows + n)
        Xd, latd, kd, yd = _dev(X), _dev(lat), _dev(keys), _dev(y)
        mu, v = _stored(Xd, latd, ld, w_off, b_col, kd, d, rows, n, intercept)
        tau = _thresholds(T, mu)
        got = _fused(Xd, yd, latd, ld, w_off, b_col, kd, d, rows, n, intercept, tau)
        want = R.confusion(mu, v, y, tau)
        assert np.array_equal(got, want), (d, rows, n, intercept, T, got, want)
        assert (got[2 + 2 * T:] == 0).all()                               # the unused threshold slots
        if T:
            strictly = R.confusion(mu, v, y, [np.nextafter(np.float32(tau[0]), np.float32(2.0))])
            assert (strictly[2] + strictly[3]).sum() < (got[2] + got[3]).sum()   # the threshold is hit exactly somewhere: >=, not >
        if T == 4:
            assert np.array_equal(got[4], np.full(n, (y == 1).sum())) and np.array_equal(got[5], np.full(n, (y == 0).sum()))   # tau = 0
            assert np.array_equal(got[6], ((mu == 1.0) & (y[None] == 1)).sum(1)) and (got[8:] == 0).all()                    # tau = 1, NaN
        again = _fused(Xd, yd, latd, ld, w_off, b_col, kd, d, rows, n, intercept, tau)
        assert got.tobytes() == again.tobytes()
        if n > 1:   # a draw's counts depend neither on the other draws, nor on n, nor on ld
            one = _fused(Xd, yd, _dev(lat[n - 1:]), ld, w_off, b_col, _dev(keys[n - 1:]), d, rows, 1, intercept, tau)
            assert np.array_equal(one[:, 0], got[:, n - 1])


def test_counts_across_the_strip_boundary_do_not_depend_on_the_strip_count(gpu):
    """rows = 128 x 513 + 1: 514 row tiles, two per strip at the default cap of 512, the last strip one tile of one row."""
    lib = L.load()
    d, rows, n = 1, 128 * 513 + 1, 3
    X, lat, ld, w_off, b_col, keys, y = _problem(d, rows, n, False, 5)
    Xd, latd, kd, yd = _dev(X), _dev(lat), _dev(keys), _dev(y)
    mu, v = _stored(Xd, latd, ld, w_off, b_col, kd, d, rows, n, False)
    tau = _thresholds(4, mu)
    want = R.confusion(mu, v, y, tau)
    got = _fused(Xd, yd, latd, ld, w_off, b_col, kd, d, rows, n, False, tau)
    assert np.array_equal(got, want)
    try:
        for cap in (1, 7, 513, 65535):
            assert lib.d3p_predict_confusion_set_strips(cap) == 0
            other = _fused(Xd, yd, latd, ld, w_off, b_col, kd, d, rows, n, False, tau)
            assert other.tobytes() == got.tobytes(), cap
    finally:
        assert lib.d3p_predict_confusion_set_strips(0) == 0


def test_a_nan_weight_counts_every_row_of_its_draw_as_nan_and_nothing_else(gpu):
    d, rows, n = 4, 300, 5
    X, lat, ld, w_off, b_col, keys, y = _problem(d, rows, n, True, 9)
    clean = lat.copy()
    lat[2, w_off + 1] = np.nan
    Xd, kd, yd = _dev(X), _dev(keys), _dev(y)
    mu, v = _stored(Xd, _dev(lat), ld, w_off, b_col, kd, d, rows, n, True)
    assert np.isnan(mu[2]).all() and (v[2] == 0).all()                    # uniform < NaN is false: the stored label is 0
    tau = [0.5, 0.0, 1.0, NAN]
    got = _fused(Xd, yd, _dev(lat), ld, w_off, b_col, kd, d, rows, n, True, tau)
    assert np.array_equal(got, R.confusion(mu, v, y, tau))
    assert got[1].tolist() == [0, 0, rows, 0, 0] and (got[2:, 2] == 0).all() and got[0, 2] == (y == 0).sum()
    base = _fused(Xd, yd, _dev(clean), ld, w_off, b_col, kd, d, rows, n, True, tau)
    keep = [0, 1, 3, 4]
    assert np.array_equal(got[:, keep], base[:, keep])


def test_c_entry_refuses_before_any_launch_and_leaves_out_alone(gpu):
    lib = L.load()
    d, rows, n = 3, 50, 4
    X, lat, ld, w_off, b_col, keys, y = _problem(d, rows, n, False, 1)
    Xd, latd, kd, yd = _dev(X), _dev(lat), _dev(keys), _dev(y)
    out = torch.full((10 * n + 1,), -123, dtype=torch.int64, device=DEV)
    tau = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5)
    s = L.stream_ptr()

    def call(ms, rows_=rows, d_=d, T=1, X_=Xd, y_=yd, out_=out, out_off=0, y_off=0, tau_=tau):
        return lib.d3p_predict_confusion(s, C.byref(ms), L.ptr(X_), C.c_void_p(y_.data_ptr() + y_off), rows_, d_, L.ptr(latd), ld, w_off, b_col, n,
                                         L.ptr(kd), tau_, T, C.c_void_p(out_.data_ptr() + out_off))

    ok = _model_struct(d, False)
    assert call(ok, rows_=0) == -1 and b"rows must be" in lib.d3p_last_error()
    assert call(ok, d_=d + 1) == -1
    assert call(ok, T=5) == -1 and b"thresholds" in lib.d3p_last_error()
    assert call(ok, tau_=None) == -1 and b"tau" in lib.d3p_last_error()
    assert call(ok, out_off=4) == -1 and b"aligned to 8" in lib.d3p_last_error()
    assert call(ok, y_off=2) == -1 and b"aligned to 4" in lib.d3p_last_error()
    assert call(ok, y_=torch.zeros(rows)) == -1 and b"device memory" in lib.d3p_last_error()          # a host pointer
    assert call(ok, X_=torch.zeros(rows, d)) == -1 and call(ok, out_=torch.zeros(10 * n, dtype=torch.int64)) == -1
    for fam in (L.D3P_FAMILY_LINREG, L.D3P_FAMILY_POISSON, L.D3P_FAMILY_GAUSS_MEAN):
        assert call(L.LogregModel(d, 0, 1.0, 1.0, 1.0, 1.0, fam, L.D3P_GUIDE_SOFTPLUS, 1.0)) == -3
    torch.cuda.synchronize()
    assert bool((out == -123).all())                                      # nothing was launched, nothing zeroed
    assert call(ok, T=0, tau_=None) == 0                                  # no thresholds need no tau
    torch.cuda.synchronize()
    assert int(out[10 * n]) == -123 and bool((out[2 * n:10 * n] == 0).all()) and not bool((out[:n] == -123).any())


# ------------------------------------------------------------------------------- the Python layer
def _guide_params(guide, d, rng):
    p = logreg_params(guide, d, True, rng)
    for name in p:                                       # predictors of moderate size: the outcomes vary
        if name.endswith("_loc"):
            p[name] = (np.asarray(p[name]) * 0.3).astype(np.float32)
    return p


def _mean_rows_of(X, w, b):
    n, d = w.shape
    lat = torch.cat([w.reshape(n, d), b.reshape(n, 1)], dim=1).contiguous()
    mu = torch.empty((n, X.shape[0]), dtype=torch.float32, device=DEV)
    ms = _model_struct(d, True)
    L.check(L.load().d3p_predict_mean_rows(L.stream_ptr(), C.byref(ms), L.ptr(X), X.shape[0], L.ptr(lat), d + 1, 0, d, n, L.ptr(mu), X.shape[0]))
    return np_(mu)


def _assert_counts(c, want, rows, y, tau, shape):
    T = len(tau)
    assert c.n_rows == rows and c.n_pos == int((y == 1).sum()) and c.n_neg == rows - c.n_pos and c.thresholds == tuple(tau)
    for x, shp in ((c.agree, shape), (c.n_nan, shape), (c.tp, shape + (T,)), (c.fp, shape + (T,))):
        assert x.dtype == torch.int64 and x.is_cuda and tuple(x.shape) == shp
    assert np.array_equal(np_(c.agree).reshape(-1), want[0]) and np.array_equal(np_(c.n_nan).reshape(-1), want[1])
    for j in range(T):
        assert np.array_equal(np_(c.tp).reshape(-1, T)[:, j], want[2 + 2 * j]) and np.array_equal(np_(c.fp).reshape(-1, T)[:, j], want[3 + 2 * j])


@pytest.mark.parametrize("guide_cls", [AutoDiagonalNormal, DiagonalNormalGuide])
def test_python_layer_equals_the_counts_of_the_samples(gpu, guide_cls):
    rng = np.random.default_rng(41)
    d, rows, n = 5, 300, 33
    Xd = _dev(rng.uniform(-1, 1, size=(rows, d)).astype(np.float32))
    y = (rng.random(size=rows) < 0.5).astype(np.float32)
    model = LogisticRegression(d, intercept=True)
    guide = guide_cls(model)
    params = _guide_params(guide, d, rng)
    k, tau = key(77), (0.5, 0.25, float(np.float32(0.9)))
    res = Ps.posterior_predictive_samples(k, n, model, (Xd,), guide, params)
    latents, counts = CL.posterior_predictive_confusion(k, n, model, (Xd, y), guide, params, thresholds=tau)
    assert set(latents) == {"w", "intercept"}
    assert torch.equal(latents["w"], res["w"]) and torch.equal(latents["intercept"].reshape(n), res["intercept"].reshape(n))   # bit for bit
    obs = np_(res["obs"])
    assert np.array_equal(np_(counts.agree), (obs == y[None].astype(np.int32)).sum(1))                 # the sampled agreement, by value
    mu = _mean_rows_of(Xd, res["w"], res["intercept"])
    _assert_counts(counts, R.confusion(mu, obs, y, tau), rows, y, tau, (n,))
    # the derived values are float64 functions of the counts
    tp, fp = np_(counts.tp), np_(counts.fp)
    assert np.array_equal(np_(counts.sampled_accuracy), np_(counts.agree) / np.float64(rows))
    assert np.array_equal(np_(counts.accuracy), (tp + (counts.n_neg - fp)) / np.float64(rows))
    assert np.array_equal(np_(counts.tpr), tp / np.float64(counts.n_pos)) and np.array_equal(np_(counts.fpr), fp / np.float64(counts.n_neg))
    assert counts.accuracy.dtype == torch.float64 and tuple(counts.f1.shape) == (n, 3)
    # given samples: predictive_samples' key rule for the sampled labels; the thresholded counts take no key
    K = key(78)
    given = CL.predictive_confusion(K, model, res, Xd, y, thresholds=tau)
    _assert_counts(given, R.confusion(mu, np_(Ps.predictive_samples(K, model, res, Xd)), y, tau), rows, y, tau, (n,))
    assert torch.equal(given.tp, counts.tp) and torch.equal(given.fp, counts.fp)
    one = {"w": res["w"][2], "intercept": res["intercept"].reshape(n)[2]}
    single = CL.predictive_confusion(K, model, one, Xd, torch.as_tensor(y).to(DEV), thresholds=tau)
    _assert_counts(single, R.confusion(mu[2:3], np_(Ps.predictive_samples(K, model, one, Xd)).reshape(1, rows), y, tau), rows, y, tau, ())
    none = CL.predictive_confusion(K, model, res, Xd, y, thresholds=())
    assert tuple(none.tp.shape) == (n, 0) and torch.equal(none.agree, given.agree)


# ------------------------------------------------------------------------------- the curve against the restatement
def _curve_c(p, y, B):
    """d3p_binary_curve on tables and a workspace that held 0xFF bytes: (hist, calib, summary) as numpy / a list of ints."""
    lib = L.load()
    pd, yd = _dev(np.asarray(p, np.float32)), _dev(np.asarray(y, np.int32))
    hist = torch.full((2, R.BINS), -1, dtype=torch.int32, device=DEV)
    calib = torch.full((3, B), -1, dtype=torch.int64, device=DEV)
    summary = torch.full((6,), -1, dtype=torch.int64, device=DEV)
    nbytes = lib.d3p_binary_curve_workspace()
    ws = torch.full((nbytes + 8,), 0xFF, dtype=torch.uint8, device=DEV)
    L.check(lib.d3p_binary_curve(L.stream_ptr(), L.ptr(pd), L.ptr(yd), len(p), B, L.ptr(hist), L.ptr(calib), L.ptr(summary), L.ptr(ws), nbytes))
    assert bool((ws[nbytes:] == 0xFF).all())                             # nothing past the workspace
    return np_(hist).astype(np.int64), np_(calib), [int(v) for v in np_(summary)]


def _assert_curve(p, y, B):
    hist, calib, summary = _curve_c(p, y, B)
    want = R.curve(p, y, B)
    assert np.array_equal(hist, want[0]) and np.array_equal(calib, want[1]) and summary == want[2], (len(p), B, summary, want[2])
    again = _curve_c(p, y, B)
    assert again[0].tobytes() == hist.tobytes() and again[1].tobytes() == calib.tobytes() and again[2] == summary
    return summary


def _scores(rng, rows, scale):
    t = rng.normal(size=rows) * scale
    p = (1.0 / (1.0 + np.exp(-t))).astype(np.float32)
    return p, (rng.random(size=rows) < p).astype(np.int32)


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 4097])
def test_curve_equals_the_restatement_on_random_scores(gpu, rows):
    rng = np.random.default_rng(rows)
    for scale, B in ((1.0, 10), (8.0, 64), (3.0, 1)):                   # (scale 8: scores pile up at both ends)
        p, y = _scores(rng, rows, scale)
        _assert_curve(p, y, B)


def test_curve_over_more_rows_than_one_pass_of_the_grid(gpu):
    """2048 workgroups of 256 rows make one pass; 300 rows more reach the loop's second turn and its partial last wavefront."""
    rng = np.random.default_rng(2)
    p, y = _scores(rng, 2048 * 256 + 300, 8.0)
    s = _assert_curve(p, y, 10)
    lo, mid, hi = R.auc_bounds(s)
    assert lo <= R.exact_auc(p, y) <= hi and hi - lo < 1e-3


def test_curve_of_repeated_and_edge_scores(gpu):
    ones = np.ones(4097, np.float32)
    y = (np.arange(4097) % 3 == 0).astype(np.int32)
    s = _assert_curve(ones, y, 10)                                        # one bin: the wavefront pre-aggregation path
    assert s == [0, 1366, 2731, 0, 1366 * 2731, 0]
    _assert_curve(np.zeros(4097, np.float32), y, 10)
    s = _assert_curve(np.full(130, -0.0, np.float32), y[:130], 7)        # -0.0f counts as 0
    assert s[3] == 0 and s[4] == s[1] * s[2]
    mixed = np.concatenate([np.zeros(50, np.float32), np.full(50, -0.0, np.float32)])
    hist, calib, _ = _curve_c(mixed, np.zeros(100, np.int32), 5)
    assert hist[0, 0] == 100 and calib[0, 0] == 100 and calib[2, 0] == 0
    half = np.array([0x3EFFFFFF, 0x3F000000, 0x3F000001], np.uint32).view(np.float32)      # 0.5f and its two neighbours
    p = np.tile(half, 40)
    _assert_curve(p, (np.arange(120) % 2).astype(np.int32), 2)
    _assert_curve(p, (np.arange(120) % 2).astype(np.int32), 64)
    edges = np.array([0, 1, 0x00800000, 0x3F7FFFFF, 0x3F800000, 0x3E800000, 0x3F400000], np.uint32).view(np.float32)   # denormal .. 1
    _assert_curve(np.tile(edges, 10), (np.arange(70) % 2).astype(np.int32), 64)


def test_curve_with_one_class_absent_and_with_invalid_rows(gpu):
    rng = np.random.default_rng(6)
    p, _ = _scores(rng, 200, 2.0)
    for label in (0, 1):
        s = _assert_curve(p, np.full(200, label, np.int32), 10)
        assert s[1] * s[2] == 0 and s[3] == 0 and s[4] == 0
        c = CL.binary_curve(_dev(p), np.full(200, label), bins=10)
        assert np.isnan(c.auc) and np.isnan(c.auc_lo) and np.isnan(c.auc_hi) and np.isnan(c.ks) and (c.n_pos, c.n_neg) == ((200, 0) if label else (0, 200))
    bad = p.copy()
    bad[[3, 64, 130]] = [np.nan, -0.25, 1.5]
    y = (rng.random(size=200) < 0.5).astype(np.int32)
    y[[7, 64]] = [2, -1]                                                 # (row 64 is invalid twice and counted once)
    s = _assert_curve(bad, y, 10)
    assert s[0] == 4 and s[1] + s[2] == 196
    with pytest.raises(ValueError, match="3 of 200 scores"):
        CL.binary_curve(_dev(bad), np.where((y == 0) | (y == 1), y, 0), bins=10)
    with pytest.raises(ValueError, match="labels must be 0 or 1"):
        CL.binary_curve(_dev(p), y, bins=10)


def test_binary_curve_derives_auc_ks_and_calibration_from_the_tables(gpu):
    rng = np.random.default_rng(8)
    p, y = _scores(rng, 5000, 3.0)
    c = CL.binary_curve(_dev(p), y, bins=12)
    hist, calib, summary = R.curve(p, y, 12)
    assert c.hist.dtype == torch.int32 and c.hist.is_cuda and np.array_equal(np_(c.hist), hist) and np.array_equal(np_(c.calib), calib)
    assert [c.n_pos, c.n_neg, c.pairs_concordant, c.pairs_same_bin] == summary[1:5] and c.bins == 12
    lo, mid, hi = R.auc_bounds(summary)
    assert (c.auc_lo, c.auc, c.auc_hi) == (lo, mid, hi) and lo <= R.exact_auc(p, y) <= hi
    assert c.ks == R.ks_statistic(hist, c.n_pos, c.n_neg) == summary[5] / (float(c.n_pos) * float(c.n_neg)) and (c.ece, c.mce) == R.calibration_errors(calib, 5000)
    assert 0.0 < c.ece < 0.05 and 0.7 < c.auc < 0.95 and 0.3 < c.ks < 0.8      # labels drawn at these scores: calibrated, informative
    fpr, tpr = c.roc()
    occupied = (hist.sum(0) > 0).sum()
    assert fpr.dtype == torch.float64 and fpr.is_cuda and fpr.numel() == tpr.numel() == occupied + 1
    f, t = np_(fpr), np_(tpr)
    assert f[0] == 0.0 and t[0] == 0.0 and f[-1] == 1.0 and t[-1] == 1.0 and np.all(np.diff(f) >= 0) and np.all(np.diff(t) >= 0)
    assert abs(np.max(np.abs(t - f)) - c.ks) <= 2.0 ** -51          # two quotients and a difference against one quotient, values <= 1
    trapezoid = float(np.sum(np.diff(f) * (t[1:] + t[:-1]) / 2.0))
    assert abs(trapezoid - c.auc) <= 4 * len(f) * np.finfo(np.float64).eps       # the same pair counts, summed in float64
    full = c.roc(compact=False)
    assert full[0].numel() == R.BINS + 1 and float(full[1][-1]) == 1.0


# ------------------------------------------------------------------------------- the report
def _example():
    path = os.path.join(ROOT, "examples", "logistic_regression.py")
    spec = importlib.util.spec_from_file_location("logistic_regression_classification_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_report_equals_the_examples_accuracy_and_the_moments_mean(gpu):
    rng = np.random.default_rng(13)
    d, rows, n = 4, 300, 20
    Xd = _dev(rng.uniform(-1, 1, size=(rows, d)).astype(np.float32))
    model = LogisticRegression(d, intercept=True)
    guide = AutoDiagonalNormal(model)
    params = _guide_params(guide, d, rng)
    w_true = rng.normal(size=d)
    y = _dev((rng.random(size=rows) < 1.0 / (1.0 + np.exp(-(np_(Xd) @ w_true)))).astype(np.float32))
    k = key(21)
    rep = CL.classification_report(k, n, model, (Xd, y), guide, params, thresholds=(0.5, 0.3), bins=8)
    # the example's number: the agreement count of the stored label matrix for the same key
    from d3p_amd.modelling import sample_multi_posterior_predictive
    samples = sample_multi_posterior_predictive(k, n, model, (Xd,), guide, (Xd,), params)
    count = int((samples["obs"] == y.to(torch.int32)).sum())
    assert int(rep.counts.agree.sum()) == count
    assert np.array_equal(np_(rep.counts.agree), np_((samples["obs"] == y.to(torch.int32)).sum(dim=1)))
    per_draw = np_(rep.counts.sampled_accuracy)
    assert rep.sampled_accuracy[0] == float(per_draw.mean())
    # mean of n correctly rounded quotients against the one quotient: (n + 2) roundings of 2^-53 each, relative
    assert abs(rep.sampled_accuracy[0] - count / (n * rows)) <= (n + 2) * 2.0 ** -53
    # estimate_accuracy itself is a float32 mean of n rows < 2^24 zeros and ones: an exact sum, then at most two float32 roundings
    acc = _example().estimate_accuracy(Xd, y, model, guide, params, k, n)
    assert abs(acc - count / (n * rows)) <= 2.0 ** -23
    assert rep.sampled_accuracy[1] == float(per_draw.std(ddof=1)) and rep.sampled_accuracy[2] <= rep.sampled_accuracy[0] <= rep.sampled_accuracy[3]
    assert len(rep.accuracy) == 2 and rep.accuracy[0][0] == float(np_(rep.counts.accuracy)[:, 0].mean())
    # the curve's input is posterior_predictive_moments' mean for the same key and n, bit for bit
    mean = PR.posterior_predictive_moments(k, n, model, (Xd, y), guide, params)["mean"]
    assert torch.equal(rep.mean_probability.view(torch.int32), mean.view(torch.int32))
    hist, calib, summary = R.curve(np_(mean), np_(y), 8)
    assert np.array_equal(np_(rep.curve.hist), hist) and np.array_equal(np_(rep.curve.calib), calib)
    assert [rep.curve.n_pos, rep.curve.n_neg, rep.curve.pairs_concordant, rep.curve.pairs_same_bin] == summary[1:5]
    # ... and the two calls drew the same latents: the mean over the report's draws of the stored mu, in float64, rounds to that mean up
    # to the one float32 rounding the moments kernel makes (a tie may fall the other way: one ulp of a value <= 1)
    assert torch.equal(rep.latents["w"], samples["w"])
    mu = _mean_rows_of(Xd, rep.latents["w"], rep.latents["intercept"])
    assert np.max(np.abs(mu.astype(np.float64).mean(0) - np_(mean).astype(np.float64))) <= 2.0 ** -23
    assert rep.n_draws == n and rep.n_rows == rows
    lines = rep.lines()
    assert len(lines) == 4 and lines[0].startswith(f"classification report ({rows} rows, {n} draws): sampled accuracy")
    assert lines[1].startswith("at threshold 0.5: accuracy") and lines[2].startswith("at threshold 0.3: accuracy") and lines[3].startswith("auc ")
    again = CL.classification_report(k, n, model, (Xd, y), guide, params, thresholds=(0.5, 0.3), bins=8)
    assert torch.equal(again.counts.agree, rep.counts.agree) and torch.equal(again.counts.tp, rep.counts.tp) and again.curve[2:] == rep.curve[2:]


def test_example_prints_the_classification_report(gpu, capsys):
    """examples/logistic_regression.py --classification-report 20 on a small table: one epoch of training, then the report's lines.
    --predictive-accuracy keeps its line."""
    import argparse
    mod = _example()
    mod.main(argparse.Namespace(sigma=0.5, num_epochs=1, learning_rate=1e-2, batch_size=200, dimensions=4, num_samples=2000, guide="auto",
                                predictive_accuracy=True, classification_report=20))
    lines = capsys.readouterr().out.splitlines()
    assert sum(l.startswith("avg accuracy on test set with found posterior (100 posterior-predictive draws):") for l in lines) == 1
    at = [i for i, l in enumerate(lines) if l.startswith("classification report (2000 rows, 20 draws): sampled accuracy")]
    assert len(at) == 1
    body = lines[at[0] + 1:at[0] + 3]
    assert body[0].startswith("at threshold 0.5: accuracy") and "TPR" in body[0] and "FPR" in body[0] and "F1" in body[0]
    assert body[1].startswith("auc ") and "KS" in body[1] and "ECE" in body[1]
    auc = float(body[1].split()[1])
    lo, hi = (float(x.strip("[],")) for x in body[1].split()[2:4])
    assert lo <= auc <= hi and 0.0 <= lo and hi <= 1.0
