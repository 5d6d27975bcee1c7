"""d3p_amd.discrepancy on the GPU: d3p_predict_discrepancy against the CPU restatement (tests/discrepancy_ref.py) of the matrices the
sibling entries store -- mu from d3p_predict_mean_rows, v from d3p_predict_glm / d3p_predict_logreg on the same arguments -- at every
edge of the tiling and for the special values; the Python layer against the *_samples calls; what the check means; the workspace
contract; the C refusals.  Every comparison is BY VALUE (NaN equal to NaN), never within a tolerance."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from d3p_amd import _lib as L
from d3p_amd import discrepancy as D
from d3p_amd import predictive as Ps
from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, LinearRegression, LogisticRegression, MeanFieldGuide,
                            PoissonRegression)

from . import discrepancy_ref as R
from . import workspace_harness as H
from .predictive_ref import key, logreg_params, np_

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FAMILIES = {"linear": L.D3P_FAMILY_LINREG, "poisson": L.D3P_FAMILY_POISSON, "logistic": L.D3P_FAMILY_LOGREG}
SIGMA = 0.75


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _model_struct(family, d, intercept):
    return L.LogregModel(d, int(intercept), 1.0, 1.0, 1.0, 1.0, FAMILIES[family], L.D3P_GUIDE_SOFTPLUS, SIGMA if family == "linear" else 0.0)


def _problem(family, d, rows, n, intercept, seed):
    """X, the latent buffer (n, ld) with a padded ld, the weights at w_off and the intercept at b_col, random obs keys, and y of the
    family's kind.  The predictors have a spread of about 2: Poisson rates on both sides of 10, sigmoids from 0.01 to 0.99."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, size=(rows, d)).astype(np.float32)
    ld, w_off, b_col = d + 3, 2, (0 if intercept else -1)
    lat = rng.normal(size=(n, ld)).astype(np.float32)
    lat[:, w_off:w_off + d] *= np.float32(4.0 / np.sqrt(d))
    if intercept:
        lat[:, b_col] = rng.uniform(-1, 2, size=n).astype(np.float32)
    keys = rng.integers(0, 2 ** 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
    if family == "linear":
        y = rng.normal(size=rows).astype(np.float32)
    elif family == "poisson":
        y = rng.poisson(3.0, size=rows).astype(np.float32)
    else:
        y = (rng.random(size=rows) < 0.5).astype(np.float32)
    return X, lat, ld, w_off, b_col, keys, y


def _stored(family, Xd, latd, ld, w_off, b_col, kd, d, rows, n, intercept):
    """(mu, v) as numpy: what d3p_predict_mean_rows and d3p_predict_glm / d3p_predict_logreg store for these arguments."""
    lib = L.load()
    ms = _model_struct(family, d, intercept)
    mu = torch.empty((n, rows), dtype=torch.float32, device=DEV)
    L.check(lib.d3p_predict_mean_rows(L.stream_ptr(), C.byref(ms), L.ptr(Xd), rows, L.ptr(latd), ld, w_off, b_col, n, L.ptr(mu), rows))
    obs = torch.empty((n, rows), dtype=torch.float32 if family == "linear" else torch.int32, device=DEV)
    if family == "logistic":
        L.check(lib.d3p_predict_logreg(L.stream_ptr(), L.ptr(Xd), rows, d, L.ptr(latd), ld, w_off, b_col, n, L.ptr(kd), L.ptr(obs)))
    else:
        L.check(lib.d3p_predict_glm(L.stream_ptr(), C.byref(ms), L.ptr(Xd), rows, d, L.ptr(latd), ld, w_off, b_col, n, L.ptr(kd), L.ptr(obs)))
    return np_(mu), np_(obs)


def _fused(family, Xd, yd, latd, ld, w_off, b_col, kd, d, rows, n, intercept, shift):
    lib = L.load()
    out = torch.empty((6, n), dtype=torch.float64, device=DEV)
    nbytes = lib.d3p_predict_discrepancy_workspace(rows, n)
    assert nbytes == R.strips(rows)[2] * 6 * n * 8
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    ms = _model_struct(family, d, intercept)
    L.check(lib.d3p_predict_discrepancy(L.stream_ptr(), C.byref(ms), L.ptr(Xd), L.ptr(yd), rows, d, L.ptr(latd), ld, w_off, b_col, n, L.ptr(kd),
                                        shift, L.ptr(out), L.ptr(ws), nbytes))
    return np_(out)


# ------------------------------------------------------------------------------- the C entry against the restatement
# d on both sides of a K slice, rows and draws on both sides of a tile, with and without an intercept; the last reaches per = 2
CASES = [(1, 1, 1, False), (32, 33, 33, False), (33, 128, 129, True), (1, 129, 33, True), (32, 300, 129, False), (33, 129, 33, False),
         (1, 65537, 3, False)]


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("d,rows,n,intercept", CASES)
def test_c_entry_equals_the_restatement_of_the_stored_matrices(gpu, family, d, rows, n, intercept):
    X, lat, ld, w_off, b_col, keys, y = _problem(family, d, rows, n, intercept, 31 * d + 7 * rows + n)
    Xd, latd, kd, yd = _dev(X), _dev(lat), _dev(keys), _dev(y)
    mu, v = _stored(family, Xd, latd, ld, w_off, b_col, kd, d, rows, n, intercept)
    shift = 1.375
    got = _fused(family, Xd, yd, latd, ld, w_off, b_col, kd, d, rows, n, intercept, shift)
    want = R.discrepancy(family, mu, v, y, shift, SIGMA)
    assert np.isfinite(want).all()
    for k in range(6):
        assert R.same(got[k], want[k]), (family, d, rows, n, intercept, k, got[k], want[k])
    again = _fused(family, Xd, yd, latd, ld, w_off, b_col, kd, d, rows, n, intercept, shift)
    assert np.array_equal(_bits(got), _bits(again))
    if n > 1:   # a draw's bits depend neither on the other draws, nor on n, nor on ld
        packed = np.ascontiguousarray(lat[n - 1:, :])
        one = _fused(family, Xd, yd, _dev(packed), ld, w_off, b_col, _dev(keys[n - 1:]), d, rows, 1, intercept, shift)
        assert np.array_equal(_bits(one[:, 0]), _bits(got[:, n - 1]))
        wide = np.full((n, ld + 5), 7.0, np.float32)
        wide[:, :ld] = lat
        assert np.array_equal(_bits(_fused(family, Xd, yd, _dev(wide), ld + 5, w_off, b_col, kd, d, rows, n, intercept, shift)), _bits(got))


def test_poisson_predictors_cover_both_branches_of_the_outcome_rule(gpu):
    """The case (32, 300, 129): rates below 10 (inversion) and above (rejection) both occur, and the replicated chi-square sees both.
    The predictor is a sum of 32 terms U(-1, 1) N(0, 1) 4 / sqrt(32): mean 0, variance 16 / 3 (sd 2.31), so a share of Phi(log 7 / 2.31)
    = 0.80 of the 38 700 rates lies below 7 and 1 - Phi(log 14 / 2.31) = 0.13 above 14; asserted: more than 0.05 on either side."""
    d, rows, n = 32, 300, 129
    X, lat, ld, w_off, b_col, keys, y = _problem("poisson", d, rows, n, False, 31 * d + 7 * rows + n)
    mu, v = _stored("poisson", _dev(X), _dev(lat), ld, w_off, b_col, _dev(keys), d, rows, n, False)
    assert (mu < 7.0).mean() > 0.05 and (mu > 14.0).mean() > 0.05
    assert v[mu < 7.0].max() > 0 and (v[mu > 14.0] != np.floor(mu[mu > 14.0])).any()


def test_poisson_special_values_enter_through_one_draw_each(gpu):
    """Draw 0: a NaN weight -- every output of draw 0 is NaN.  Draw 1: its second weight is -200 and column 1 of X is 1 in rows 3 and 70
    only, so the rate of those two rows underflows to mu == 0 (V == 0): against y = 0 the row contributes nothing, against y = 1 +inf.
    The replicate of such a row is 0: matched.  Every other draw's bits are those of the run without the special latent rows."""
    d, rows, n = 2, 130, 5
    rng = np.random.default_rng(17)
    X = np.zeros((rows, d), np.float32)
    X[:, 0] = rng.uniform(-1, 1, size=rows)
    X[[3, 70], 1] = 1.0
    lat = rng.normal(size=(n, d)).astype(np.float32)
    clean = lat.copy()
    lat[0, 0] = np.nan
    lat[1, 1] = -200.0
    keys = rng.integers(0, 2 ** 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
    y = rng.poisson(1.0, size=rows).astype(np.float32)
    y[3], y[70] = 0.0, 1.0
    Xd, kd = _dev(X), _dev(keys)
    run = lambda la, yy: _fused("poisson", Xd, _dev(yy), _dev(la), d, 0, -1, kd, d, rows, n, False, 0.5)
    got = run(lat, y)
    mu, v = _stored("poisson", Xd, _dev(lat), d, 0, -1, kd, d, rows, n, False)
    assert np.isnan(mu[0]).all() and (v[0] == -1).all() and mu[1, 3] == 0.0 and mu[1, 70] == 0.0 and v[1, 3] == 0 and v[1, 70] == 0
    assert R.same(got, R.discrepancy("poisson", mu, v, y, 0.5))
    assert np.isnan(got[:, 0]).all()
    assert got[0, 1] == np.inf and np.isfinite(got[1:, 1]).all()
    y0 = y.copy()
    y0[70] = 0.0                                       # both underflowed rows matched: a finite realized discrepancy
    got0 = run(lat, y0)
    assert np.isfinite(got0[:, 1]).all() and R.same(got0, R.discrepancy("poisson", mu, v, y0, 0.5))
    base = run(clean, y)
    assert np.isfinite(base).all()
    assert np.array_equal(_bits(got[:, 2:]), _bits(base[:, 2:]))


def test_logistic_saturated_predictors_reach_zero_variance_on_both_sides(gpu):
    """One weight, X = 1: draws at t = +40 and +200 have mu == 1.0 exactly (V == 0 from above).  At t = -40 the two-branch sigmoid
    gives mu = exp(-40) > 0 (V = mu: tiny, not 0: a label of 1 gives a finite 1 / mu); V == 0 from below needs exp(t) to underflow, t =
    -200.  A matched label contributes nothing, the other one +inf; the replicate of a saturated row is its mean: matched."""
    rows, n = 40, 5
    X = np.ones((rows, 1), np.float32)
    lat = np.array([[40.0], [-40.0], [200.0], [-200.0], [0.3]], np.float32)
    keys = np.random.default_rng(1).integers(0, 2 ** 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
    Xd, latd, kd = _dev(X), _dev(lat), _dev(keys)
    mu, v = _stored("logistic", Xd, latd, 1, 0, -1, kd, 1, rows, n, False)
    assert (mu[0] == 1.0).all() and (mu[2] == 1.0).all() and (mu[3] == 0.0).all() and (mu[1] > 0.0).all() and (mu[1] < 1e-17).all()
    assert (v[0] == 1).all() and (v[2] == 1).all() and (v[3] == 0).all()
    for label in (0.0, 1.0):
        y = np.full(rows, label, np.float32)
        got = _fused("logistic", Xd, _dev(y), latd, 1, 0, -1, kd, 1, rows, n, False, 0.25)
        assert R.same(got, R.discrepancy("logistic", mu, v, y, 0.25))
        hit, miss = ((0, 2), (3,)) if label == 1.0 else ((3,), (0, 2))
        assert all(got[0, s] == 0.0 for s in hit) and all(got[0, s] == np.inf for s in miss)
        assert got[1, 0] == 0.0 and got[1, 2] == 0.0 and got[1, 3] == 0.0 and np.isfinite(got[:, 4]).all()
        assert np.isfinite(got[0, 1]) and (got[0, 1] > 1e17 if label == 1.0 else got[0, 1] < 1e-15)


# ------------------------------------------------------------------------------- the Python layer
def _family_model(family, d, intercept):
    if family == "linear":
        return LinearRegression(d, intercept=intercept, obs_scale=SIGMA)
    return PoissonRegression(d, intercept=intercept) if family == "poisson" else LogisticRegression(d, intercept=intercept)


def _guide_params(guide, d, rng):
    p = logreg_params(guide, d, True, rng)
    for name in p:                                       # predictors of moderate size: every family's outcomes vary
        if name.endswith("_loc"):
            p[name] = (np.asarray(p[name]) * 0.3).astype(np.float32)
    return p


def _mean_rows_of(family, X, w, b):
    """d3p_predict_mean_rows of the latents (w (n, d), b (n,)) packed afresh: (n, rows) float32 as numpy."""
    n, d = w.shape
    lat = torch.cat([w.reshape(n, d), b.reshape(n, 1)], dim=1).contiguous()
    mu = torch.empty((n, X.shape[0]), dtype=torch.float32, device=DEV)
    ms = _model_struct(family, d, True)
    L.check(L.load().d3p_predict_mean_rows(L.stream_ptr(), C.byref(ms), L.ptr(X), X.shape[0], L.ptr(lat), d + 1, 0, d, n, L.ptr(mu), X.shape[0]))
    return np_(mu)


def _assert_sums(sums, want, rows, shift, shape):
    assert sums.n_rows == rows and sums.shift == shift
    for k, x in enumerate(sums._six()):
        assert x.dtype == torch.float64 and x.is_cuda and tuple(x.shape) == shape
        assert R.same(np_(x).reshape(-1), want[k]), k


def _outcomes_for(family, rng, rows):
    if family == "linear":
        return rng.normal(size=rows).astype(np.float32)
    return (rng.poisson(2.0, size=rows) if family == "poisson" else (rng.random(size=rows) < 0.5)).astype(np.float32)


@pytest.mark.parametrize("family,guide_cls", [(f, g) for f in FAMILIES for g in (AutoDiagonalNormal, DiagonalNormalGuide)]
                         + [("logistic", MeanFieldGuide)])
def test_python_layer_equals_the_restatement_of_the_samples(gpu, family, guide_cls):
    rng = np.random.default_rng(41)
    d, rows, n = 5, 300, 33
    Xd = _dev(rng.uniform(-1, 1, size=(rows, d)).astype(np.float32))
    y = _outcomes_for(family, rng, rows)
    model = _family_model(family, d, True)
    guide = guide_cls(model)
    params = _guide_params(guide, d, rng)
    k, shift = key(77), 0.75
    res = Ps.posterior_predictive_samples(k, n, model, (Xd,), guide, params)
    latents, sums = D.posterior_predictive_discrepancy(k, n, model, (Xd, y), guide, params, shift=shift)
    assert set(latents) == {"w", "intercept"}
    assert torch.equal(latents["w"], res["w"]) and torch.equal(latents["intercept"].reshape(n), res["intercept"].reshape(n))   # bit for bit
    mu = _mean_rows_of(family, Xd, res["w"], res["intercept"])
    want = R.discrepancy(family, mu, np_(res["obs"]), y, shift, SIGMA)
    _assert_sums(sums, want, rows, shift, (n,))
    assert sums.model is model
    # shift=None: float32(mean(y))
    auto = D.posterior_predictive_discrepancy(k, n, model, (Xd, y), guide, params)[1]
    assert auto.shift == float(np.float32(_dev(y).mean().item()))
    _assert_sums(auto, R.discrepancy(family, mu, np_(res["obs"]), y, auto.shift, SIGMA), rows, auto.shift, (n,))
    # given samples: predictive_samples' key rule for the replicate; the outputs that take no key are the posterior call's, bit for bit
    K = key(78)
    given = D.predictive_discrepancy(K, model, res, Xd, y, shift=shift)
    want_given = R.discrepancy(family, mu, np_(Ps.predictive_samples(K, model, res, Xd)), y, shift, SIGMA)
    _assert_sums(given, want_given, rows, shift, (n,))
    for a, b in zip(given._six()[:1] + given._six()[2:], sums._six()[:1] + sums._six()[2:]):
        assert torch.equal(H.raw_bytes(a), H.raw_bytes(b))
    one = {"w": res["w"][2], "intercept": res["intercept"].reshape(n)[2]}
    single = D.predictive_discrepancy(K, model, one, Xd, y, shift=shift)
    v_one = np_(Ps.predictive_samples(K, model, one, Xd))
    _assert_sums(single, R.discrepancy(family, mu[2], v_one, y, shift, SIGMA), rows, shift, ())
    # the derived values are float64 functions of the six
    assert np.array_equal(np_(sums.mean_mu), shift + want[2] / rows)
    assert np.array_equal(np_(sums.var_fit()), (want[3] - want[2] * want[2] / rows) / (rows - 1))
    assert np.array_equal(np_(sums.rmse), np.sqrt(want[5] / rows)) and np.array_equal(np_(sums.bias), want[4] / rows)
    var_res = (want[5] - want[4] * want[4] / rows) / (rows - 1)
    var_fit = np_(sums.var_fit())
    assert np.array_equal(np_(sums.bayes_r2("residual")), var_fit / (var_fit + var_res))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_replicated_row_checked_against_itself(gpu, family):
    """y = draw 0's own replicated row: the realized and the replicated discrepancy of draw 0 are the same sum of the same terms."""
    rng = np.random.default_rng(5)
    d, rows, n = 4, 257, 20
    Xd = _dev(rng.uniform(-1, 1, size=(rows, d)).astype(np.float32))
    model = _family_model(family, d, True)
    guide = AutoDiagonalNormal(model)
    params = _guide_params(guide, d, rng)
    k = key(3)
    y = Ps.posterior_predictive_samples(k, n, model, (Xd,), guide, params)["obs"][0]
    _, sums = D.posterior_predictive_discrepancy(k, n, model, (Xd, y.to(torch.float32)), guide, params)
    obs, rep = np_(sums.chi2_obs), np_(sums.chi2_rep)
    assert np.isfinite(obs).all() and obs[0] == rep[0] and obs[0] > 0.0
    res = D.discrepancy_check(k, n, model, (Xd, y.to(torch.float32)), guide, params)
    assert res.n_draws == n and res.n_rows == rows and res.n_nonfinite == 0
    assert np.array_equal(res.chi2_obs, obs) and np.array_equal(res.chi2_rep, rep) and res.chi2_obs.dtype == np.float64
    assert res.p_ge == (rep >= obs).sum() / n and res.p_le == (rep <= obs).sum() / n and res.p_ge >= 1 / n and res.p_le >= 1 / n
    assert np.array_equal(res.dispersion, obs / rows) and set(res.r2) == {"residual", "model"}
    for x in (res.r2["residual"], res.r2["model"], res.rmse, res.bias):
        assert x.shape == (n,) and np.isfinite(x).all()
    assert len(res.lines()) == 8


def test_check_finds_zero_inflation_in_a_poisson_fit(gpu):
    """2000 rows at a predictor near 2 (rate 7.4), latents one weight vector with 1e-3 jitter, every second y overwritten with 0: the
    realized chi-square is near 1000 + 1000 x 7.4 against 2000 +- 65 for a replicate (margins for any key: tests/test_discrepancy_host.py,
    test_zero_inflation_margin_on_the_cpu)."""
    rng = np.random.default_rng(8)
    d, rows, n = 4, 2000, 50
    X = rng.uniform(-1, 1, size=(rows, d)).astype(np.float32)
    model = PoissonRegression(d, intercept=True)
    guide = AutoDiagonalNormal(model)
    params = {"auto_loc": np.array([0.01, -0.01, 0.02, 0.0, 2.0], np.float32), "auto_scale": np.full(5, 1e-3, np.float32)}
    y = Ps.posterior_predictive_samples(key(1), 1, model, (X,), guide, params)["obs"][0].clone()
    y[::2] = 0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = D.discrepancy_check(key(2), n, model, (X, y), guide, params)
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)]
    assert res.p_ge == 0.0 and res.p_le == 1.0 and res.n_nonfinite == 0
    assert res.chi2_obs.min() > 2.0 * res.chi2_rep.max()
    assert res.dispersion.min() > 2.0
    assert any("p_ge 0.000" in line for line in res.lines())


def test_check_counts_and_reports_draws_that_are_not_finite(gpu):
    d, rows, n = 2, 40, 6
    X = np.zeros((rows, d), np.float32)
    X[:, 0] = 1.0
    X[7, 0] = 100.0                                      # predictor -100 w_0: the rate underflows to 0 where w_0 is near 2
    model = PoissonRegression(d)
    guide = AutoDiagonalNormal(model)
    params = {"auto_loc": np.array([-2.0, 0.0], np.float32), "auto_scale": np.full(2, 1e-3, np.float32)}
    with pytest.warns(RuntimeWarning, match="not finite"):
        res = D.discrepancy_check(key(4), n, model, (X, np.ones(rows, np.float32)), guide, params)
    assert res.n_nonfinite == n and (res.chi2_obs == np.inf).all() and np.isfinite(res.chi2_rep).all() and res.p_ge == 0.0 and res.p_le == 1.0


def test_linear_model_r2_is_var_fit_over_var_fit_plus_sigma_squared(gpu):
    rng = np.random.default_rng(9)
    d, rows, n = 3, 500, 16
    X = rng.uniform(-1, 1, size=(rows, d)).astype(np.float32)
    model = LinearRegression(d, intercept=True, obs_scale=SIGMA)
    guide = AutoDiagonalNormal(model)
    params = {"auto_loc": np.array([1.0, -0.5, 0.25, 0.1], np.float32), "auto_scale": np.full(4, 0.05, np.float32)}
    y = (X @ np.array([1.0, -0.5, 0.25], np.float32) + 0.1 + SIGMA * rng.normal(size=rows)).astype(np.float32)
    _, sums = D.posterior_predictive_discrepancy(key(5), n, model, (X, y), guide, params)
    s, ss = np_(sums.mu_sum), np_(sums.mu_sumsq)
    var_fit = (ss - s * s / rows) / (rows - 1)
    sigma2 = np.float64(np.float32(SIGMA)) ** 2
    assert np.array_equal(np_(sums.bayes_r2("model")), var_fit / (var_fit + sigma2))
    r2 = np_(sums.bayes_r2("model"))
    assert ((r2 > 0.2) & (r2 < 0.6)).all()               # var_fit near (1 + 0.25 + 0.0625) / 3 = 0.44 against sigma^2 = 0.5625
    assert 0.8 < float(sums.dispersion.mean()) < 1.2      # y was drawn at this sigma: the chi-square is near its rows


# ------------------------------------------------------------------------------- the workspace contract
def _under_fill(fill, fn):
    rec = H.Recorder(fill, 0, None)
    mp = pytest.MonkeyPatch()
    H.guarded_empty(mp, D, rec, "discrepancy")
    try:
        st = fn()
        torch.cuda.synchronize()
    finally:
        mp.undo()
    rec.check_all(fill)
    assert len(rec.workspaces) == 1 and rec.workspaces[0].nbytes == R.strips(st.n_rows)[2] * 6 * st.chi2_obs.numel() * 8
    return [H.raw_bytes(x) for x in st._six()]


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_entry_ignores_what_the_workspace_held_and_stays_inside_it(gpu, family):
    rng = np.random.default_rng(12)
    d, rows, n = 3, 1000, 130                            # 8 strips, two draw tiles
    model = _family_model(family, d, True)
    X = _dev(rng.uniform(-1, 1, size=(rows, d)).astype(np.float32))
    y = _dev(_outcomes_for(family, rng, rows))
    samples = {"w": _dev(rng.normal(size=(n, d)).astype(np.float32)), "intercept": _dev(rng.normal(size=n).astype(np.float32))}
    k = key(6)
    fn = lambda: D.predictive_discrepancy(k, model, samples, X, y, shift=0.5)
    base = _under_fill("zero", fn)
    for fill in ("ones", "big", "bits"):
        got = _under_fill(fill, fn)
        assert all(torch.equal(a, b) for a, b in zip(base, got)), (family, fill)


# ------------------------------------------------------------------------------- refusals at the C boundary
def test_c_entry_refuses_before_any_launch_and_leaves_outputs_and_workspace_alone(gpu):
    lib = L.load()
    d, rows, n = 3, 50, 4
    X, lat, ld, w_off, b_col, keys, y = _problem("linear", d, rows, n, False, 1)
    Xd, latd, kd, yd = _dev(X), _dev(lat), _dev(keys), _dev(y)
    out = torch.full((6, n), -123.0, dtype=torch.float64, device=DEV)
    nbytes = lib.d3p_predict_discrepancy_workspace(rows, n)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    s = L.stream_ptr()

    def call(ms, rows_=rows, nb=nbytes, d_=d, shift=0.0, X_=Xd, y_=yd, out_=out, ws_=ws, out_off=0, ws_off=0, y_off=0):
        return lib.d3p_predict_discrepancy(s, C.byref(ms), L.ptr(X_), C.c_void_p(y_.data_ptr() + y_off), rows_, d_, L.ptr(latd), ld, w_off, b_col, n,
                                           L.ptr(kd), shift, C.c_void_p(out_.data_ptr() + out_off), C.c_void_p(ws_.data_ptr() + ws_off), nb)

    ok = _model_struct("linear", d, False)
    assert call(ok, nb=nbytes - 1) == -1 and b"workspace" in lib.d3p_last_error()
    assert call(ok, ws_off=4, nb=nbytes - 4) == -1 and b"workspace" in lib.d3p_last_error()
    assert call(ok, ws_=torch.zeros(nbytes, dtype=torch.uint8)) == -1 and b"device memory" in lib.d3p_last_error()
    assert call(ok, rows_=0) == -1 and b"rows must be" in lib.d3p_last_error()
    assert call(ok, d_=d + 1) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(ok, shift=bad) == -1 and b"finite" in lib.d3p_last_error()
    assert call(ok, out_off=4) == -1 and b"aligned to 8" in lib.d3p_last_error()
    assert call(ok, y_off=2) == -1 and b"aligned to 4" in lib.d3p_last_error()
    assert call(ok, y_=torch.zeros(rows)) == -1 and b"device memory" in lib.d3p_last_error()          # a host pointer
    assert call(ok, X_=torch.zeros(rows, d)) == -1 and call(ok, out_=torch.zeros(6, n, dtype=torch.float64)) == -1
    gauss = L.LogregModel(d, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_GAUSS_MEAN, L.D3P_GUIDE_SOFTPLUS, 1.0)
    assert call(gauss) == -3 and b"Gaussian-mean" in lib.d3p_last_error()
    sites = L.LogregModel(d, 1, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LOGREG, L.D3P_GUIDE_EXP_SITES, 0.0)
    assert call(sites) == -3 and b"D3P_GUIDE_EXP_SITES" in lib.d3p_last_error()
    bad_sigma = L.LogregModel(d, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LINREG, L.D3P_GUIDE_SOFTPLUS, 0.0)
    assert call(bad_sigma) == -1
    torch.cuda.synchronize()
    assert bool((out == -123.0).all()) and bool((ws == 0x5A).all())       # nothing was launched
    assert call(ok) == 0                                                  # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert not bool((out == -123.0).any())


# ------------------------------------------------------------------------------- the example flag
def test_poisson_example_prints_the_check_of_its_zero_inflated_counts(gpu, capsys):
    """examples/poisson_regression.py --zero-inflate 0.5 --discrepancy 20 on a small table.  Half of the counts are forced to 0: a row
    whose untouched count has rate lambda then has mean lambda / 2 and variance lambda / 2 + lambda^2 / 4.  A Poisson fit follows the
    means, mu near lambda / 2, where the row's expected realized term is 1 + lambda / 2 against 1 for a replicate; with lambda =
    exp(N(0, 1)), mean 1.65, the realized chi-square of 2000 rows lies near 3600 against 2000 +- 100 for a replicate, so the paired
    share is 0 and the dispersion above 1."""
    import argparse
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "poisson_regression.py")
    spec = importlib.util.spec_from_file_location("poisson_regression_discrepancy_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(argparse.Namespace(sigma=0.5, clip_threshold=1.0, num_steps=300, learning_rate=2e-2, batch_size=200, dimensions=4,
                                num_samples=2000, discrepancy=20, zero_inflate=0.5))
    lines = capsys.readouterr().out.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("realized discrepancy check (2000 rows, 20 draws)")]
    assert len(at) == 1
    body = lines[at[0] + 1:at[0] + 9]
    assert body[0].startswith("discrepancy chi2") and "p_ge 0.000" in body[0] and "p_le 1.000" in body[0]
    by_name = {b.split()[1]: b.split() for b in body[1:]}
    assert list(by_name) == ["chi2_obs", "chi2_rep", "dispersion", "r2_residual", "r2_model", "rmse", "bias"]
    assert float(by_name["dispersion"][2]) > 1.0
