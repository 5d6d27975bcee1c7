"""d3p_amd.infer_util on the device against tests/loglik_ref.py: float64 on the CPU, the bound |dll/dt| band_t + link_tol per element
(band_t from tests/predictive_ref.py, link_tol calibrated on the CPU: tests/test_loglik_host.py), the lppd bound on top of it.
-inf is compared by equality, NaN never passes.  Sizes are the smallest that cross the kernel's tile edges (draw tile 128, row tile
128, K slice 32, half-wave 32)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import loglik_ref as LR
from tests import predictive_ref as P

pytestmark = pytest.mark.gpu


def np_(t):
    return t.detach().cpu().numpy()


def make_model(family, d, intercept, **kw):
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    if family == "logistic":
        return LogisticRegression(d, intercept=intercept)
    if family == "linear":
        return LinearRegression(d, intercept=intercept, obs_scale=kw.pop("sigma", LR.SIGMA["linear"]))
    return PoissonRegression(d, intercept=intercept, **kw)


def samples_of(W, b):
    s = {"w": torch.tensor(W).cuda()}
    if b is not None:
        s["intercept"] = torch.tensor(b).cuda()
    return s


# ---------------------------------------------------------------- tile-edge sweep
@pytest.mark.parametrize("family,n,rows,d,intercept", LR.sweep_cases())
def test_both_forms_at_tile_edges(gpu, family, n, rows, d, intercept):
    from d3p_amd import infer_util as U
    X, y, W, b = LR.inputs(family, n, rows, d, intercept)
    sigma = LR.SIGMA[family]
    assert np.abs(LR.linear_predictor(X, W, b)).max() <= 4.0
    ll = LR.ll64(family, X, y, W, b, sigma)
    bound = LR.ll_bound(family, X, y, W, b, sigma, ll)
    lppd = LR.lppd64(ll)
    assert np.isfinite(ll).all()
    model = make_model(family, d, intercept)
    Xt, yt = torch.tensor(X).cuda(), torch.tensor(y).cuda()
    what = f"{family} n={n} rows={rows} d={d} intercept={intercept}"
    got = U.log_likelihood(model, samples_of(W, b), Xt, yt, rows)
    assert list(got) == ["obs"] and got["obs"].shape == (n, rows) and got["obs"].dtype == torch.float32
    LR.assert_close(np_(got["obs"]), ll, bound, what + " rows form")
    dens = U.log_predictive_density(model, samples_of(W, b), Xt, yt, rows)
    assert dens.shape == (rows,) and dens.dtype == torch.float32
    LR.assert_close(np_(dens), lppd, LR.lppd_bound(ll, bound, lppd), what + " lppd form")
    if n == 1:      # a single sample: w of shape (d,) gives (rows,), the same bits
        one = {"w": torch.tensor(W[0]).cuda()}
        if b is not None:
            one["intercept"] = float(b[0])
        single = U.log_likelihood(model, one, Xt, yt)["obs"]
        assert single.shape == (rows,) and torch.equal(single, got["obs"][0])


# ---------------------------------------------------------------- the two forms against each other
@pytest.mark.parametrize("family", LR.FAMILIES)
def test_lppd_form_is_the_logsumexp_of_the_rows_form(gpu, family):
    """n = 257: three draw tiles, so the online merge and both waves' combination run."""
    from d3p_amd import infer_util as U
    n, rows, d = 257, 300, 33
    X, y, W, b = LR.inputs(family, n, rows, d, True, seed=91)
    model = make_model(family, d, True)
    Xt, yt, s = torch.tensor(X).cuda(), torch.tensor(y).cuda(), samples_of(W, b)
    ll_dev = np_(U.log_likelihood(model, s, Xt, yt)["obs"]).astype(np.float64)
    dens = np_(U.log_predictive_density(model, s, Xt, yt)).astype(np.float64)
    assert np.isfinite(ll_dev).all()
    exp = LR.lppd64(ll_dev)
    LR.assert_close(dens, exp, LR.LPPD_EXTRA * np.maximum(1.0, np.abs(exp)), f"{family}: lppd form against its own rows form")


# ---------------------------------------------------------------- Poisson overflow
def _overflow_problem(all_draws):
    """d = 4, rows = 70, n = 5.  One draw: w of draw 2 is scaled so that its nine largest t reach 95 and above; the other rows of X are turned away from that w
    so that every other element stays moderate (a finite ll of -exp(76) would make the bounds vacuous).  Every draw: the first 10 rows of
    X are set to 200 u / |u|^2, u the mean draw, so that t is about 200 under each draw."""
    n, rows, d = 5, 70, 4
    X, y, W, b = LR.inputs("poisson", n, rows, d, False, seed=5)
    X, W = X.copy(), W.copy()
    if all_draws:
        u = W.astype(np.float64).mean(axis=0)
        X[:10] = (200.0 * u / (u @ u)).astype(np.float32)
    else:
        w2 = W[2].astype(np.float64)
        t = X.astype(np.float64) @ w2
        c = 95.0 / np.sort(t)[-9]                           # the nine largest t of draw 2 reach 95 and above ...
        low = (t < np.sort(t)[-9]) & (c * np.abs(t) > 4.0)  # ... and on the other rows X gives up enough of w2's direction for c t to stay at 4
        X[low] = (X[low].astype(np.float64) - ((1.0 - 4.0 / (c * np.abs(t[low]))) * t[low] / (w2 @ w2))[:, None] * w2).astype(np.float32)
        W[2] = (W[2] * np.float32(c)).astype(np.float32)
    t = LR.linear_predictor(X, W, None)
    assert not ((t > 80.0) & (t < 89.0)).any()      # nothing near float32's overflow point 88.72: no element can fall on the other side
    return n, rows, d, X, y, W, t


def test_poisson_overflow_in_one_draw(gpu):
    from d3p_amd import infer_util as U
    n, rows, d, X, y, W, t = _overflow_problem(False)
    ll = LR.ll64("poisson", X, y, W, None, 1.0)
    over = t > 89.0
    assert over[2].any() and not over[[0, 1, 3, 4]].any() and np.array_equal(np.isneginf(ll), over)   # the comparator is where the test means it
    lppd = LR.lppd64(ll)
    assert np.isfinite(lppd).all()
    rest = np.delete(ll, 2, axis=0)
    hit = over[2]
    assert np.allclose(lppd[hit], LR.logsumexp_rows(rest)[hit] - np.log(n), rtol=1e-13)          # ... over the remaining draws
    model = make_model("poisson", d, False)
    Xt, yt, s = torch.tensor(X).cuda(), torch.tensor(y).cuda(), samples_of(W, None)
    got = np_(U.log_likelihood(model, s, Xt, yt)["obs"])
    bound = LR.ll_bound("poisson", X, y, W, None, 1.0, ll)
    LR.assert_close(got, ll, bound, "poisson overflow, rows form")
    assert np.all(np.isneginf(got[over]))
    dens = np_(U.log_predictive_density(model, s, Xt, yt))
    assert np.isfinite(dens).all()
    LR.assert_close(dens, lppd, LR.lppd_bound(ll, bound, lppd), "poisson overflow, lppd form")


def test_poisson_overflow_in_every_draw_is_minus_inf_not_nan(gpu):
    from d3p_amd import infer_util as U
    n, rows, d, X, y, W, t = _overflow_problem(True)
    ll = LR.ll64("poisson", X, y, W, None, 1.0)
    lppd = LR.lppd64(ll)
    dead = (t > 89.0).all(axis=0)
    assert dead.any() and not dead.all() and np.array_equal(np.isneginf(lppd), dead) and not np.isnan(lppd).any()
    model = make_model("poisson", d, False)
    Xt, yt, s = torch.tensor(X).cuda(), torch.tensor(y).cuda(), samples_of(W, None)
    bound = LR.ll_bound("poisson", X, y, W, None, 1.0, ll)
    LR.assert_close(np_(U.log_likelihood(model, s, Xt, yt)["obs"]), ll, bound, "poisson overflow everywhere, rows form")
    dens = np_(U.log_predictive_density(model, s, Xt, yt))
    assert not np.isnan(dens).any() and np.all(np.isneginf(dens[dead]))
    LR.assert_close(dens, lppd, LR.lppd_bound(ll, bound, lppd), "poisson overflow everywhere, lppd form")


# ---------------------------------------------------------------- key rule
@pytest.mark.parametrize("guide_name", ["auto", "mean_field"])
def test_posterior_density_draws_the_latents_of_the_predictive(gpu, guide_name):
    """Same key, same n: the latents are sample_multi_posterior_predictive's, the kernel is the same -- bit for bit."""
    from d3p_amd import infer_util as U
    from d3p_amd import modelling as M
    from d3p_amd.models import AutoDiagonalNormal, LogisticRegression, MeanFieldGuide
    d, n, rows = 33, 130, 200
    model = LogisticRegression(d, intercept=True)
    guide = AutoDiagonalNormal(model) if guide_name == "auto" else MeanFieldGuide(model)
    r = np.random.default_rng(12)
    params = {k: torch.tensor(v) for k, v in P.logreg_params(guide, d, True, r).items()}
    X = torch.tensor((r.normal(size=(rows, d)) / np.sqrt(d)).astype(np.float32)).cuda()
    y = torch.tensor((r.random(rows) < 0.5).astype(np.float32)).cuda()
    key = P.key(77)
    res = M.sample_multi_posterior_predictive(key, n, model, (X,), guide, (X,), params)
    exp = U.log_predictive_density(model, {"w": res["w"], "intercept": res["intercept"]}, X, y)
    got = U.posterior_log_predictive_density(key, n, model, (X, y, rows), guide, params)
    assert got.shape == (rows,) and bool(torch.isfinite(got).all())
    assert torch.equal(got, exp)
    other = U.posterior_log_predictive_density(P.key(78), n, model, (X, y), guide, params)
    assert not torch.equal(other, got)


# ---------------------------------------------------------------- views and buffers
@pytest.mark.parametrize("family", LR.FAMILIES)
def test_separate_strided_samples_give_the_packed_buffers_bits(gpu, family):
    from d3p_amd import infer_util as U
    n, rows, d = 131, 150, 33
    X, y, W, b = LR.inputs(family, n, rows, d, True, seed=3)
    model = make_model(family, d, True)
    Xt, yt = torch.tensor(X).cuda(), torch.tensor(y).cuda()
    packed = torch.tensor(np.concatenate([W, b[:, None]], axis=1)).cuda()
    view = {"w": packed[:, :d], "intercept": packed[:, d]}
    assert U._packed_view(view["w"], view["intercept"], n, d)[0].data_ptr() == packed.data_ptr()      # read in place
    wide = torch.zeros((n, 2 * d), device="cuda")
    wide[:, ::2] = torch.tensor(W).cuda()
    tall = torch.zeros((3 * n,), device="cuda")
    tall[::3] = torch.tensor(b).cuda()
    apart = {"w": wide[:, ::2], "intercept": tall[::3]}
    assert not apart["w"].is_contiguous() and not apart["intercept"].is_contiguous()
    assert U._packed_view(apart["w"], apart["intercept"], n, d) is None
    host = {"w": W, "intercept": b.reshape(n, 1)}                                                       # numpy arrays, (n, 1)
    for f in (lambda s: U.log_likelihood(model, s, Xt, yt)["obs"], lambda s: U.log_predictive_density(model, s, Xt, yt)):
        ref = f(view)
        assert torch.equal(f(apart), ref) and torch.equal(f(host), ref)


def _struct(family, d, intercept, guide=0, sigma=0.5):
    import d3p_amd._lib as L
    fam = {"logistic": L.D3P_FAMILY_LOGREG, "linear": L.D3P_FAMILY_LINREG, "poisson": L.D3P_FAMILY_POISSON, "gauss": L.D3P_FAMILY_GAUSS_MEAN}[family]
    return L.LogregModel(d, int(intercept), 1.0, 1.0, 1.0, 1.0, fam, guide, sigma)


@pytest.mark.parametrize("family", LR.FAMILIES)
def test_outputs_stay_inside_their_buffers(gpu, family):
    """Canary values around both outputs, at sizes that end inside a tile."""
    import d3p_amd._lib as L
    from d3p_amd import infer_util as U
    lib = L.load()
    n, rows, d, pad = 129, 130, 5, 512
    X, y, W, b = LR.inputs(family, n, rows, d, True, seed=8)
    Xt, yt = torch.tensor(X).cuda(), torch.tensor(y).cuda()
    lat = torch.tensor(np.concatenate([W, b[:, None]], axis=1)).cuda()
    ms = _struct(family, d, True, sigma=LR.SIGMA[family])
    for lppd, size in ((0, n * rows), (1, rows)):
        buf = torch.full((size + 2 * pad,), 12345.0, device="cuda")
        out = buf[pad:pad + size]
        fn = lib.d3p_loglik_lppd if lppd else lib.d3p_loglik_rows
        L.check(fn(L.stream_ptr(), C.byref(ms), L.ptr(Xt), L.ptr(yt), rows, L.ptr(lat), d + 1, 0, d, n, L.ptr(out)))
        torch.cuda.synchronize()
        assert bool((buf[:pad] == 12345.0).all()) and bool((buf[pad + size:] == 12345.0).all())
        assert not bool((out == 12345.0).any())
        s = {"w": lat[:, :d], "intercept": lat[:, d]}
        model = make_model(family, d, True)
        ref = U.log_predictive_density(model, s, Xt, yt) if lppd else U.log_likelihood(model, s, Xt, yt)["obs"].reshape(-1)
        assert torch.equal(out, ref)


# ---------------------------------------------------------------- C entries
def test_c_entries_refuse_and_accept_as_declared(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    d, n, rows = 3, 2, 4
    X, y, lat = torch.zeros((rows, d), device="cuda"), torch.zeros(rows, device="cuda"), torch.zeros((n, d + 1), device="cuda")
    out = torch.full((n * rows,), 7.0, device="cuda")

    def call(fn, ms, X_=X, y_=y, lat_=lat, out_=out, rows_=rows, n_=n, b_col=None):
        b_col = (d if ms.intercept else -1) if b_col is None else b_col
        return fn(L.stream_ptr(), C.byref(ms), L.ptr(X_), L.ptr(y_), rows_, L.ptr(lat_), d + 1, 0, b_col, n_, L.ptr(out_))
    for fn in (lib.d3p_loglik_rows, lib.d3p_loglik_lppd):
        assert call(fn, _struct("gauss", d, False)) == -3                                   # D3P_E_UNSUPPORTED
        assert call(fn, _struct("logistic", d, True, guide=L.D3P_GUIDE_EXP_SITES)) == -3
        assert call(fn, _struct("poisson", d, True, guide=L.D3P_GUIDE_EXP)) == 0            # (the transform is not read otherwise)
        for kw in ({"X_": None}, {"y_": None}, {"lat_": None}, {"out_": None}, {"n_": 0}):
            assert call(fn, _struct("linear", d, True), **kw) == -1, kw                     # D3P_E_INVALID_ARG
        assert call(fn, _struct("linear", 0, True)) == -1
        assert call(fn, _struct("linear", d, True), b_col=-1) == -1 and call(fn, _struct("linear", d, False), b_col=d) == -1
        out.fill_(7.0)
        assert call(fn, _struct("logistic", d, True), rows_=0) == 0                         # D3P_OK, nothing launched
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    with pytest.raises(ValueError, match="null X / y / latent / out"):
        L.check(call(lib.d3p_loglik_rows, _struct("linear", d, True), out_=None))


# ---------------------------------------------------------------- end to end
def test_trained_linear_regression_scores_held_out_rows_better(gpu):
    """The surface composes: DPSVI.run_steps -> get_params -> posterior_log_predictive_density.  Not a calibration."""
    import d3p_amd.random as rng
    from d3p_amd import infer_util as U
    from d3p_amd.minibatch import subsample_batchify_data
    from d3p_amd.models import Adam, AutoDiagonalNormal, LinearRegression, Trace_ELBO
    from d3p_amd.svi import DPSVI, DPSVIState
    d, N, held = 4, 2000, 500
    r = np.random.default_rng(0)
    w_true = np.array([1.0, -0.7, 0.4, 0.2])
    Xall = r.normal(size=(N + held, d)).astype(np.float32)
    yall = (Xall @ w_true + 0.5 * r.normal(size=N + held)).astype(np.float32)
    Xt, yt = torch.tensor(Xall[:N]).cuda(), torch.tensor(yall[:N]).cuda()
    Xh, yh = torch.tensor(Xall[N:]).cuda(), torch.tensor(yall[N:]).cuda()
    model = LinearRegression(d, obs_scale=0.5)
    guide = AutoDiagonalNormal(model)
    svi = DPSVI(model, guide, Adam(2e-2), Trace_ELBO(), 1.0, 0.5, num_obs_total=N)
    start = torch.tensor(np.concatenate([np.zeros(d, np.float32), np.full(d, -2.0, np.float32)]), device="cuda")
    st = DPSVIState(svi.optim.init(start), rng.PRNGKey(3), float(N))
    init, get_batch = subsample_batchify_data((Xt, yt), 200)
    _, bstate = init(rng.PRNGKey(4))
    trained, losses = svi.run_steps(st, get_batch, bstate, 0, 300)
    assert bool(torch.isfinite(losses).all())
    key = P.key(9)
    before = U.posterior_log_predictive_density(key, 64, model, (Xh, yh, held), guide, svi.get_params(st))
    after = U.posterior_log_predictive_density(key, 64, model, (Xh, yh, held), guide, svi.get_params(trained))
    assert before.shape == after.shape == (held,) and bool(torch.isfinite(before).all()) and bool(torch.isfinite(after).all())
    print(f"mean held-out lppd: {float(before.mean()):.4f} at the initial parameters, {float(after.mean()):.4f} after 300 steps")
    assert float(after.mean()) > float(before.mean())
