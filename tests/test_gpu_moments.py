"""d3p_amd.prediction on the device against tests/moments_ref.py: float64 on the CPU, per-row bounds derived there (the float32
product's band and the link's rounding, calibrated on the CPU, propagated through the mean and the variance).  Non-finite entries are
compared by their class.  Sizes are the smallest that cross the kernel's tile edges (draw tile 128, row tile 128, K slice 32,
half-wave 32) and the draw counts at which the second wave of a row block owns no draw, and one."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import moments_ref as MR
from tests import predictive_ref as P

LR = MR.LR
pytestmark = pytest.mark.gpu


def np_(t):
    return t.detach().cpu().numpy()


def np_both(res):
    return {k: np_(v) for k, v in res.items()}


def make_model(family, d, intercept, sigma=None):
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    if family == "logistic":
        return LogisticRegression(d, intercept=intercept)
    if family == "linear":
        return LinearRegression(d, intercept=intercept, obs_scale=MR.SIGMA["linear"] if sigma is None else sigma)
    return PoissonRegression(d, intercept=intercept)


def samples_of(W, b):
    s = {"w": torch.tensor(W).cuda()}
    if b is not None:
        s["intercept"] = torch.tensor(b).cuda()
    return s


def run(family, X, W, b):
    from d3p_amd import prediction as Pm
    rows, d = X.shape
    res = Pm.predictive_moments(make_model(family, d, b is not None), samples_of(W, b), torch.tensor(X).cuda())
    assert sorted(res) == ["mean", "variance"]
    for v in res.values():
        assert v.shape == (rows,) and v.dtype == torch.float32 and v.is_cuda
    return np_both(res)


# ---------------------------------------------------------------- tile-edge sweep
@pytest.mark.parametrize("family,n,rows,d,intercept", MR.sweep_cases())
def test_moments_at_tile_edges(gpu, family, n, rows, d, intercept):
    X, _, W, b = LR.inputs(family, n, rows, d, intercept)
    assert np.abs(LR.linear_predictor(X, W, b)).max() <= 4.0
    got = run(family, X, W, b)
    mean, var, _, _ = MR.check(got, family, X, W, b, MR.SIGMA[family], f"{family} n={n} rows={rows} d={d} intercept={intercept}")
    assert np.isfinite(mean).all() and np.isfinite(var).all() and (got["variance"] >= 0).all()


# ---------------------------------------------------------------- the between-draw term
@pytest.mark.parametrize("family", MR.FAMILIES)
def test_identical_draws_have_no_between_draw_variance(gpu, family):
    """n = 130 (two draw tiles, both waves of a row block), rows = 129, d = 33; every draw the same latent row."""
    X, W, b = MR.identical_draws(family)
    assert W.shape == (130, 33) and X.shape == (129, 33)
    got = run(family, X, W, b)
    MR.check(got, family, X, W, b, MR.SIGMA[family], f"{family} identical draws")
    one = run(family, X, W[:1], b[:1])                                  # n = 1: mean = mu, var = v
    MR.check(one, family, X, W[:1], b[:1], MR.SIGMA[family], f"{family} n=1")
    if family == "linear":
        sig2 = np.float32(np.float64(np.float32(MR.SIGMA["linear"])) ** 2)
        assert np.all(got["variance"] == sig2) and np.all(one["variance"] == sig2)      # bitwise float32(sigma^2)
    if family == "poisson":
        assert np.array_equal(got["variance"], got["mean"]) and np.array_equal(one["variance"], one["mean"])
    if family != "logistic":
        assert np.array_equal(got["mean"], one["mean"])                 # the mean of equal values is that value
    else:
        mu, v, _, _ = MR.conditional_moments(family, LR.linear_predictor(X, W[:1], b[:1]), 1.0)
        MR.assert_close(one["variance"], v[0], MR.bounds(family, X, W[:1], b[:1], 1.0)[1], "logistic n=1: var = p (1 - p)")


# ---------------------------------------------------------------- cancellation
def test_large_mean_small_spread_keeps_the_between_draw_variance(gpu):
    """Intercept draws near 1e4 with a between-draw standard deviation of 1e-2: within the derived bound, which a float32 sum of
    squares misses by four to six orders of magnitude (tests/test_moments_host.py)."""
    X, W, b = MR.cancellation_problem()
    got = run("linear", X, W, b)
    _, var, _, b_var = MR.check(got, "linear", X, W, b, MR.SIGMA["linear"], "cancellation")
    assert np.all(b_var < 1e-3) and np.all(var - MR.SIGMA["linear"] ** 2 > 2e-5)      # the bound is about the term itself
    assert np.all(got["variance"] > np.float32(MR.SIGMA["linear"] ** 2))


# ---------------------------------------------------------------- non-finite values
def test_poisson_overflow_in_one_draw(gpu):
    X, W, t = MR.overflow_problem(False)
    over = t > 89.0
    assert over[2].any() and not over[[0, 1, 3, 4]].any()
    hit = over.any(axis=0)
    got = run("poisson", X, W, None)
    mean, var, _, _ = MR.check(got, "poisson", X, W, None, 1.0, "poisson overflow in one draw")
    assert np.array_equal(np.isposinf(mean), hit) and np.array_equal(np.isposinf(var), hit)      # the comparator is where the test means it
    assert np.all(np.isposinf(got["mean"][hit])) and np.all(np.isposinf(got["variance"][hit]))
    assert np.isfinite(got["mean"][~hit]).all() and np.isfinite(got["variance"][~hit]).all() and (~hit).sum() > 50


def test_poisson_overflow_in_every_draw_is_inf_not_nan(gpu):
    X, W, t = MR.overflow_problem(True)
    dead = (t > 89.0).all(axis=0)
    assert dead.sum() == 10
    got = run("poisson", X, W, None)
    MR.check(got, "poisson", X, W, None, 1.0, "poisson overflow in every draw")
    assert np.all(np.isposinf(got["mean"][dead])) and np.all(np.isposinf(got["variance"][dead]))
    assert not np.isnan(got["mean"]).any() and not np.isnan(got["variance"]).any()


def test_poisson_variance_beyond_float32_is_inf_beside_a_finite_mean(gpu):
    """mu of 1e30 and 3e30 in two draws: the between-draw term is 1e60 in float64 and rounds to +inf once."""
    X = np.array([[1.0], [0.0]], np.float32)
    W = np.log(np.array([[1e30], [3e30]])).astype(np.float32)
    got = run("poisson", X, W, None)
    MR.check(got, "poisson", X, W, None, 1.0, "poisson huge variance")
    assert np.isfinite(got["mean"]).all() and np.isposinf(got["variance"][0]) and got["variance"][1] == 1.0


@pytest.mark.parametrize("family", MR.FAMILIES)
def test_nan_in_one_sample_makes_every_row_nan(gpu, family):
    n, rows, d = 70, 130, 5
    X, _, W, b = LR.inputs(family, n, rows, d, True, seed=31)
    W = W.copy()
    W[66, 2] = np.nan                       # (draw 66: the second wave's)
    got = run(family, X, W, b)
    MR.check(got, family, X, W, b, MR.SIGMA[family], f"{family} NaN sample")
    assert np.isnan(got["mean"]).all() and np.isnan(got["variance"]).all()


# ---------------------------------------------------------------- key rule
@pytest.mark.parametrize("family,guide_name", [("logistic", "auto"), ("logistic", "diagonal"), ("logistic", "mean_field"),
                                               ("linear", "auto"), ("linear", "diagonal"), ("poisson", "auto"), ("poisson", "diagonal")])
def test_posterior_moments_draw_the_latents_of_the_predictive(gpu, family, guide_name):
    """Same key, same n: the latents are sample_multi_posterior_predictive's for a LogisticRegression of the same d, intercept, guide
    and params (the draws do not depend on the family), the kernel is the same -- bit for bit."""
    from d3p_amd import modelling as M
    from d3p_amd import prediction as Pm
    from d3p_amd.models import AutoDiagonalNormal, DiagonalNormalGuide, LogisticRegression, MeanFieldGuide
    d, n, rows = 33, 129, 200
    model, logi = make_model(family, d, True), LogisticRegression(d, intercept=True)
    cls = {"auto": AutoDiagonalNormal, "diagonal": DiagonalNormalGuide, "mean_field": MeanFieldGuide}[guide_name]
    guide, lguide = cls(model), cls(logi)
    r = np.random.default_rng(12)
    params = {k: torch.tensor(0.3 * v if k.endswith("_loc") else v) for k, v in P.logreg_params(lguide, d, True, r).items()}
    X = torch.tensor((r.normal(size=(rows, d)) / np.sqrt(d)).astype(np.float32)).cuda()
    y = torch.zeros(rows).cuda()
    key = P.key(77)
    res = M.sample_multi_posterior_predictive(key, n, logi, (X,), lguide, (X,), params)
    exp = Pm.predictive_moments(model, {"w": res["w"], "intercept": res["intercept"]}, X)
    got = Pm.posterior_predictive_moments(key, n, model, (X, y, rows), guide, params)
    for name in ("mean", "variance"):
        assert got[name].shape == (rows,) and got[name].dtype == torch.float32 and bool(torch.isfinite(got[name]).all())
        assert torch.equal(got[name], exp[name]), name
    other = Pm.posterior_predictive_moments(P.key(78), n, model, (X,), guide, params)
    assert not torch.equal(other["mean"], got["mean"])


# ---------------------------------------------------------------- views, buffers, reproducibility
@pytest.mark.parametrize("family", MR.FAMILIES)
def test_columns_of_one_buffer_are_read_in_place(gpu, family):
    from d3p_amd import infer_util as U
    from d3p_amd import prediction as Pm
    n, rows, d = 131, 150, 33
    X, _, W, b = LR.inputs(family, n, rows, d, True, seed=3)
    model = make_model(family, d, True)
    Xt = torch.tensor(X).cuda()
    packed = torch.tensor(np.concatenate([b[:, None], W, np.zeros((n, 2), np.float32)], axis=1)).cuda()      # [intercept | w | unused]
    view = {"w": packed[:, 1:d + 1], "intercept": packed[:, 0]}
    first, ld, w_off, b_col = U._pack(model, view, n, d)
    assert (first.data_ptr(), ld, w_off, b_col) == (packed.data_ptr(), d + 3, 1, 0)      # no copy
    ref = Pm.predictive_moments(model, view, Xt)
    apart = {"w": torch.tensor(W).cuda(), "intercept": torch.tensor(b).cuda()}           # two buffers: packed into one
    host = {"w": W, "intercept": b.reshape(n, 1)}                                           # numpy arrays, (n, 1)
    for s in (apart, host):
        res = Pm.predictive_moments(model, s, Xt)
        assert torch.equal(res["mean"], ref["mean"]) and torch.equal(res["variance"], ref["variance"])
    MR.check(np_both(ref), family, X, W, b, MR.SIGMA[family], f"{family} view")
    again = Pm.predictive_moments(model, view, Xt)                                          # two calls: the same bits
    assert torch.equal(again["mean"], ref["mean"]) and torch.equal(again["variance"], ref["variance"])


def _struct(family, d, intercept, guide=0, sigma=0.5):
    import d3p_amd._lib as L
    fam = {"logistic": L.D3P_FAMILY_LOGREG, "linear": L.D3P_FAMILY_LINREG, "poisson": L.D3P_FAMILY_POISSON, "gauss": L.D3P_FAMILY_GAUSS_MEAN}[family]
    return L.LogregModel(d, int(intercept), 1.0, 1.0, 1.0, 1.0, fam, guide, sigma)


@pytest.mark.parametrize("family", MR.FAMILIES)
def test_outputs_stay_inside_their_buffers(gpu, family):
    """Canary words before and after both outputs, rows = 129: one row into the second tile."""
    import d3p_amd._lib as L
    from d3p_amd import prediction as Pm
    lib = L.load()
    n, rows, d, pad = 129, 129, 5, 512
    X, _, W, b = LR.inputs(family, n, rows, d, True, seed=8)
    Xt = torch.tensor(X).cuda()
    lat = torch.tensor(np.concatenate([W, b[:, None]], axis=1)).cuda()
    ms = _struct(family, d, True, sigma=MR.SIGMA[family])
    bufs = [torch.full((rows + 2 * pad,), 12345.0, device="cuda") for _ in range(2)]
    mean, var = (buf[pad:pad + rows] for buf in bufs)
    L.check(lib.d3p_predict_moments(L.stream_ptr(), C.byref(ms), L.ptr(Xt), rows, L.ptr(lat), d + 1, 0, d, n, L.ptr(mean), L.ptr(var)))
    torch.cuda.synchronize()
    for buf, out in zip(bufs, (mean, var)):
        assert bool((buf[:pad] == 12345.0).all()) and bool((buf[pad + rows:] == 12345.0).all())
        assert not bool((out == 12345.0).any())
    ref = Pm.predictive_moments(make_model(family, d, True), {"w": lat[:, :d], "intercept": lat[:, d]}, Xt)
    assert torch.equal(mean, ref["mean"]) and torch.equal(var, ref["variance"])


# ---------------------------------------------------------------- C entry
def test_c_entry_refuses_and_accepts_as_declared(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    d, n, rows = 3, 2, 4
    X, lat = torch.zeros((rows, d), device="cuda"), torch.zeros((n, d + 1), device="cuda")
    mean, var = torch.full((rows,), 7.0, device="cuda"), torch.full((rows,), 7.0, device="cuda")

    def call(ms, X_=X, lat_=lat, mean_=mean, var_=var, rows_=rows, n_=n, b_col=None, ld=d + 1, w_off=0):
        b_col = (d if ms.intercept else -1) if b_col is None else b_col
        return lib.d3p_predict_moments(L.stream_ptr(), C.byref(ms), L.ptr(X_), rows_, L.ptr(lat_), ld, w_off, b_col, n_, L.ptr(mean_), L.ptr(var_))
    assert call(_struct("gauss", d, False)) == -3                                   # D3P_E_UNSUPPORTED
    assert call(_struct("logistic", d, True, guide=L.D3P_GUIDE_EXP_SITES)) == -3
    for kw in ({"X_": None}, {"lat_": None}, {"mean_": None}, {"var_": None}, {"n_": 0}, {"ld": d}, {"w_off": 2}, {"b_col": 1}):
        assert call(_struct("linear", d, True), **kw) == -1, kw                     # D3P_E_INVALID_ARG
    assert call(_struct("linear", 0, True)) == -1
    assert call(_struct("linear", d, True), b_col=-1) == -1 and call(_struct("linear", d, False), b_col=d) == -1
    for sigma in (0.0, -1.0, float("inf"), float("nan")):
        assert call(_struct("linear", d, True, sigma=sigma)) == -1, sigma
    assert call(_struct("poisson", d, True, sigma=0.0)) == 0                         # (lik_sigma is read for the linear family only)
    host = torch.zeros(rows)
    assert call(_struct("logistic", d, True), mean_=host) == -1                     # not device memory
    mean.fill_(7.0)
    var.fill_(7.0)
    assert call(_struct("logistic", d, True), rows_=0) == 0                         # D3P_OK, nothing launched
    torch.cuda.synchronize()
    assert bool((mean == 7.0).all()) and bool((var == 7.0).all())
    assert call(_struct("poisson", d, True, guide=L.D3P_GUIDE_EXP)) == 0            # (the transform is not read otherwise)
    torch.cuda.synchronize()
    assert bool((mean == 1.0).all()) and bool((var == 1.0).all())                   # exp(0) under every draw
    with pytest.raises(ValueError, match="null X / latent / mean / var"):
        L.check(call(_struct("linear", d, True), var_=None))
