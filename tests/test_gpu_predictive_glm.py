"""d3p_amd.predictive on the GPU: linear and Poisson outcomes at the tile's edges, every outcome against the CPU comparator
(tests/predictive_glm_ref.py states the restatement and every bound used here), the key rule against d3p_amd.modelling, the Poisson
rule's branches at exact rates, the outcomes' distribution, special values, views, bounds and the C entry's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from d3p_amd import _lib as L
from d3p_amd import modelling as M
from d3p_amd import predictive as Ps
from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, LinearRegression, LogisticRegression, MeanFieldGuide,
                            PoissonRegression)

from . import predictive_glm_ref as G
from .predictive_ref import assert_latent, assert_not_vacuous, key, logreg_expect, logreg_params, np_

pytestmark = pytest.mark.gpu

SIGMA = 0.75


def _model(family, d, intercept, sigma=SIGMA):
    return LinearRegression(d, intercept=intercept, obs_scale=sigma) if family == "linear" else PoissonRegression(d, intercept=intercept)


def _latents(res, n, d, intercept):
    return np_(res["w"]).reshape(n, d), (np_(res["intercept"]).reshape(n) if intercept else None)


def _check_obs(O, family, obs, X, w, b, okeys, d, what, sigma=SIGMA, exact=False):
    if family == "linear":
        assert obs.dtype == np.float32
        G.check_linear(O, obs, X, w, b, sigma, okeys, d, what)
    else:
        assert_not_vacuous(G.check_poisson(O, obs, X, w, b, okeys, d, what, exact=exact), obs.size, what)


# ------------------------------------------------------------------------------- tile edges, every outcome
@pytest.mark.parametrize("family", ["linear", "poisson"])
@pytest.mark.parametrize("d,rows,n,intercept", G.TILE_EDGES)
def test_tile_edges_every_outcome(gpu, O, family, d, rows, n, intercept):
    seed = G.edge_seed(d, rows, n, intercept)
    X, params = G.generic_problem(d, rows, n, intercept, seed)
    model = _model(family, d, intercept)
    k = key(seed)
    res = Ps.posterior_predictive_samples(k, n, model, (X,), AutoDiagonalNormal(model), params)
    assert set(res) == ({"w", "intercept", "obs"} if intercept else {"w", "obs"})
    assert tuple(res["obs"].shape) == (n, rows) and res["obs"].dtype == (torch.float32 if family == "linear" else torch.int32)
    stand_in = LogisticRegression(d, intercept=intercept)
    exp, okeys = logreg_expect(O, np_(k), n, True, stand_in, AutoDiagonalNormal(stand_in), params, X)
    w, b = _latents(res, n, d, intercept)
    lat = w if b is None else np.concatenate([w, b[:, None]], axis=1)
    for i, (loc, eps, sc) in enumerate(exp["_auto_latent"]):
        assert_latent(lat[i], loc, eps, sc, f"latent[{i}]")
    _check_obs(O, family, np_(res["obs"]), X, w, b, okeys, d, f"{family} d={d} rows={rows} n={n} intercept={intercept}")


# ------------------------------------------------------------------------------- the key rule
@pytest.mark.parametrize("guide_cls", [AutoDiagonalNormal, DiagonalNormalGuide, MeanFieldGuide])
def test_logistic_equals_modelling_bit_for_bit(gpu, guide_cls):
    rng = np.random.default_rng(5)
    d, rows, n = 33, 129, 130
    X = rng.normal(size=(rows, d)).astype(np.float32)
    model = LogisticRegression(d, intercept=True)
    guide = guide_cls(model)
    params = logreg_params(guide, d, True, rng)
    k = key(91)
    mine = Ps.posterior_predictive_samples(k, n, model, (X, None, rows), guide, params)
    ref = M.sample_multi_posterior_predictive(k, n, model, (X,), guide, (X,), params)
    assert set(mine) == {"w", "intercept", "obs"}
    for name in mine:
        assert torch.equal(mine[name].reshape(n, -1), ref[name].reshape(n, -1)), name
    sub = {"intercept": np.float32(0.25)}
    mine = Ps.prior_predictive_samples(k, n, model, (X,), sub)
    ref = M.sample_multi_prior_predictive(k, n, model, (X,), sub)
    for name in ("w", "intercept", "obs"):
        assert torch.equal(mine[name].reshape(n, -1), ref[name].reshape(n, -1)), name
    assert mine["obs"].dtype == torch.int32 and 0 < int(mine["obs"].sum()) < n * rows


@pytest.mark.parametrize("family", ["linear", "poisson"])
@pytest.mark.parametrize("guide_cls", [AutoDiagonalNormal, DiagonalNormalGuide])
def test_latents_are_the_logistic_models_and_given_samples_follow_their_own_keys(gpu, O, family, guide_cls):
    """The latents of the two newer families are sample_multi_posterior_predictive's for a LogisticRegression of the same d, intercept
    and guide, bit for bit; predictive_samples over them applies the same outcome rule with the obs keys split(K, n) (its docstring's
    relation): both results pass the comparator, each with its own keys."""
    d, rows, n, intercept = 33, 130, 129, True
    X, params = G.generic_problem(d, rows, n, intercept, 17)
    if guide_cls is DiagonalNormalGuide:
        params = {"w_loc": params["auto_loc"], "w_std_log": np.log(params["auto_scale"])}
    model, stand_in = _model(family, d, intercept), LogisticRegression(d, intercept=intercept)
    k = key(23)
    res = Ps.posterior_predictive_samples(k, n, model, (X,), guide_cls(model), params)
    ref = M.sample_multi_posterior_predictive(k, n, stand_in, (X,), guide_cls(stand_in), (X,), params)
    assert torch.equal(res["w"], ref["w"]) and torch.equal(res["intercept"].reshape(n), ref["intercept"].reshape(n))
    w, b = _latents(res, n, d, intercept)
    _, okeys = logreg_expect(O, np_(k), n, True, stand_in, guide_cls(stand_in), {p: np.asarray(v) for p, v in params.items()}, X)
    _check_obs(O, family, np_(res["obs"]), X, w, b, okeys, d, f"{family} posterior")
    K = key(24)
    given = Ps.predictive_samples(K, model, res, X)
    assert tuple(given.shape) == (n, rows) and given.dtype == res["obs"].dtype
    _check_obs(O, family, np_(given), X, w, b, list(O.tf_split(np_(K), n)), d, f"{family} given samples")
    assert not torch.equal(given, res["obs"])
    # numpy samples are packed once and give the same outcomes; a single sample is n = 1 with the key split(K, 1)[0]
    assert torch.equal(Ps.predictive_samples(K, model, {"w": w, "intercept": b}, X, None, rows), given)
    one = Ps.predictive_samples(K, model, {"w": w[3], "intercept": b[3]}, X)
    assert tuple(one.shape) == (rows,)
    _check_obs(O, family, np_(one)[None], X, w[3:4], b[3:4], list(O.tf_split(np_(K), 1)), d, f"{family} single sample")


# ------------------------------------------------------------------------------- the two-rounding rule, bit for bit
def test_linear_outcome_rounds_twice(gpu):
    """The device's eps is read through a call with w = 0, no intercept and sigma = 1 (obs = eps exactly); then, with dyadic X and w (t
    exact in float32 in any order) and the same key, obs must be float32(t) + float32(eps) * float32(sigma) bit for bit."""
    rng = np.random.default_rng(8)
    d, rows, n = 33, 129, 130
    X = (rng.integers(-2, 3, size=(rows, d)) / 2).astype(np.float32)
    w = (rng.integers(1, 9, size=d) * rng.choice([-1, 1], size=d) / 64).astype(np.float32)
    k = key(61)
    eps = np_(Ps.prior_predictive_samples(k, n, LinearRegression(d, obs_scale=1.0), (X,), {"w": np.zeros(d, np.float32)})["obs"])
    assert np.abs(eps).max() > 3 and abs(eps.mean()) < 0.05
    for sigma in (0.3, 2.7):
        got = np_(Ps.prior_predictive_samples(k, n, LinearRegression(d, obs_scale=sigma), (X,), {"w": w})["obs"])
        t = (X.astype(np.float64) @ w.astype(np.float64)).astype(np.float32)
        assert np.array_equal(t.astype(np.float64), X.astype(np.float64) @ w.astype(np.float64))
        want = t[None, :] + (eps * np.float32(sigma)).astype(np.float32)
        assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------- the Poisson rule's branches at exact rates
def test_poisson_branches_at_exact_rates(gpu, O):
    X, wv, t = G.exact_rate_problem()
    n, d = 256, X.shape[1]
    k = key(77)
    res = Ps.prior_predictive_samples(k, n, PoissonRegression(d), (X,), {"w": wv})
    obs = np_(res["obs"])
    assert np.array_equal(np_(res["w"]), np.broadcast_to(wv, (n, d)))
    w, _, okeys = G.oracle_draws(O, np_(k), n, d, False, None, X.shape[0], posterior=False, subst={"w": wv})
    for i, rate in enumerate(G.EXACT_RATES):      # equality and the vacuity cap per rate
        rws = slice(3 * i, 3 * i + 3)
        exp, judged, _ = G.judge_poisson(np.broadcast_to(t[rws], (n, 3)), 0.0, _RowsOf(G.ObsUniforms(O, okeys, X.shape[0]), rws))
        bad = judged & (obs[:, rws] != exp)
        assert not bad.any(), (rate, int(bad.sum()), obs[:, rws][bad][:5], exp[bad][:5])
        assert_not_vacuous(float((~judged).mean()), n * 3, f"rate {rate}")
        b_mean, _ = G.poisson_moment_bounds(np.exp(t[3 * i]), n * 3)
        assert abs(obs[:, rws].mean() - np.exp(t[3 * i])) <= b_mean, rate


class _RowsOf:
    def __init__(self, unif, rows):
        self.unif, self.rows = unif, rows

    def __call__(self, j, draws=None):
        U, V = self.unif(j, draws)
        return U[:, self.rows], V[:, self.rows]


# ------------------------------------------------------------------------------- distribution
def test_poisson_outcomes_have_the_rates_mean_and_variance(gpu):
    """Prior predictive with w substituted: every draw of a row has the same rate lam = expf(float32(log rate)); 4096 draws.  |mean - lam|
    <= 5 sqrt(lam / n) and the variance within 5 of its standard errors (predictive_glm_ref.poisson_moment_bounds); the device's lam is
    within 2^-22 of the float64 one, 0.24 at 1e6 against a bound of 78."""
    rates = np.array([0.5, 9.9, 10.1, 50.0, 1e4, 1e6])
    n = 4096
    X = np.log(rates).astype(np.float32).reshape(-1, 1)
    obs = np_(Ps.prior_predictive_samples(key(3), n, PoissonRegression(1), (X,), {"w": np.ones(1, np.float32)})["obs"]).astype(np.float64)
    lam = np.exp(X[:, 0].astype(np.float64))
    for r, rate in enumerate(lam):
        b_mean, b_var = G.poisson_moment_bounds(rate, n)
        mean, var = obs[:, r].mean(), obs[:, r].var(ddof=1)
        print(f"lam = {rate}: mean {mean} (bound {b_mean}), variance {var} (bound {b_var})")
        assert abs(mean - rate) <= b_mean and abs(var - rate) <= b_var
    assert obs.min() >= 0


@pytest.mark.parametrize("sigma", [0.25, 3.0])
def test_linear_noise_is_standard_normal_times_sigma(gpu, sigma):
    n, rows = 4096, 5
    X = np.zeros((rows, 2), np.float32)
    obs = np_(Ps.prior_predictive_samples(key(4), n, LinearRegression(2, obs_scale=sigma), (X,), {"w": np.ones(2, np.float32)})["obs"])
    eps = obs.astype(np.float64) / sigma
    b_mean, b_var = G.normal_moment_bounds(n)
    for r in range(rows):
        assert abs(eps[:, r].mean()) <= b_mean and abs(eps[:, r].var(ddof=1) - 1) <= b_var
    assert len(np.unique(obs)) > 0.99 * obs.size


# ------------------------------------------------------------------------------- special values
def test_poisson_special_values(gpu, O):
    """Rows (through X, with w = 1): t = -inf and an underflowing t give 0, an overflowing t gives 2147483647, NaN gives -1; the rows
    between them keep their outcomes.  Then overflow in ONE draw only (through that draw's intercept)."""
    tvals = np.array([1.0, -np.inf, 2.0, -120.0, 3.0, 100.0, 0.5, np.nan, 2.5, 89.0], np.float32)
    X = tvals.reshape(-1, 1)
    n, rows = 130, len(tvals)
    k = key(9)
    model = PoissonRegression(1)
    obs = np_(Ps.prior_predictive_samples(k, n, model, (X,), {"w": np.ones(1, np.float32)})["obs"])
    assert np.all(obs[:, [1, 3]] == 0) and np.all(obs[:, [5, 9]] == 2147483647) and np.all(obs[:, 7] == -1)
    w, _, okeys = G.oracle_draws(O, np_(k), n, 1, False, None, rows, posterior=False, subst={"w": np.ones(1, np.float32)})
    share = G.check_poisson(O, obs, X, w, None, okeys, 1, "special rows", exact=True)
    assert_not_vacuous(share, obs.size)
    fine = [0, 2, 4, 6, 8]
    assert obs[:, fine].min() >= 0 and obs[:, fine].max() < 100 and obs[:, fine].std() > 0
    # one draw overflows: samples given, intercept 100 in draw 64 (the second wave's first draw)
    b = np.zeros(n, np.float32)
    b[64] = 100.0
    Xs = np.full((129, 1), 1.0, np.float32)
    K = key(10)
    got = np_(Ps.predictive_samples(K, PoissonRegression(1, intercept=True), {"w": np.ones((n, 1), np.float32), "intercept": b}, Xs))
    assert np.all(got[64] == 2147483647) and got[np.arange(n) != 64].max() < 100
    share = G.check_poisson(O, got, Xs, np.ones((n, 1), np.float32), b, list(O.tf_split(np_(K), n)), 1, "one draw overflows", exact=True)
    assert_not_vacuous(share, got.size)


# ------------------------------------------------------------------------------- views, bounds, determinism, the C entry
def _call(ms, X, rows, d, lat, ld, w_off, b_col, n, okeys, obs):
    return L.load().d3p_predict_glm(L.stream_ptr(), C.byref(ms) if ms is not None else None, L.ptr(X), rows, d, L.ptr(lat), ld, w_off, b_col, n,
                                    L.ptr(okeys), L.ptr(obs))


def _struct(fam, d, intercept, sigma=SIGMA, guide=L.D3P_GUIDE_SOFTPLUS):
    return L.LogregModel(d, int(intercept), 1.0, 1.0, 1.0, 1.0, fam, guide, sigma)


@pytest.mark.parametrize("family", ["linear", "poisson"])
def test_views_canaries_and_determinism(gpu, family):
    """The latents are read where they lie (a buffer with the intercept BEFORE the weights and a wide row stride); nothing is written
    outside obs (canaries around it); two calls give equal bits; the module's packed views are read in place."""
    rng = np.random.default_rng(12)
    d, rows, n, ld = 33, 129, 130, 40
    fam = L.D3P_FAMILY_LINREG if family == "linear" else L.D3P_FAMILY_POISSON
    X = torch.as_tensor(rng.uniform(-1, 1, size=(rows, d)).astype(np.float32)).cuda()
    buf = torch.as_tensor(rng.uniform(-0.2, 0.2, size=(n, ld)).astype(np.float32)).cuda()
    okeys = torch.as_tensor(rng.integers(0, 2 ** 31, size=(n, 2)).astype(np.int32)).cuda()
    dt = torch.float32 if family == "linear" else torch.int32
    pad = 4096
    outs = []
    for _ in range(2):
        whole = torch.full((pad + n * rows + pad,), 12345, dtype=dt, device="cuda")
        assert _call(_struct(fam, d, True), X, rows, d, buf, ld, 5, 2, n, okeys, whole[pad:]) == 0
        torch.cuda.synchronize()
        assert bool((whole[:pad] == 12345).all()) and bool((whole[pad + n * rows:] == 12345).all())
        outs.append(whole[pad:pad + n * rows].reshape(n, rows).clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    model = _model(family, d, True)
    mine = Ps.predictive_samples(okeys[0], model, {"w": buf[:, 5:5 + d], "intercept": buf[:, 2]}, X)      # views of buf: packed in place
    copy = Ps.predictive_samples(okeys[0], model, {"w": buf[:, 5:5 + d].contiguous(), "intercept": buf[:, 2].contiguous()}, X)
    assert torch.equal(mine.view(torch.int32), copy.view(torch.int32))
    from d3p_amd.infer_util import _packed_view
    first, ld_, w_off, b_col = _packed_view(buf[:, 5:5 + d], buf[:, 2], n, d)
    assert (first.data_ptr(), ld_, w_off, b_col) == (buf[:, 2].data_ptr(), ld, 3, 0)


def test_c_entry_refusals_come_before_any_launch(gpu):
    d, rows, n = 3, 5, 4
    X = torch.zeros(rows, d, device="cuda")
    lat = torch.zeros(n, d + 1, device="cuda")
    okeys = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
    obs = torch.full((n, rows), 77, dtype=torch.int32, device="cuda")
    lin, poi = L.D3P_FAMILY_LINREG, L.D3P_FAMILY_POISSON
    INVALID, UNSUPPORTED = -1, -3

    def call(ms, X_=X, rows_=rows, d_=d, lat_=lat, ld=d + 1, w_off=0, b_col=d, n_=n, okeys_=okeys, obs_=obs):
        return _call(ms, X_, rows_, d_, lat_, ld, w_off, b_col, n_, okeys_, obs_)
    assert call(_struct(L.D3P_FAMILY_LOGREG, d, True)) == UNSUPPORTED
    assert call(_struct(L.D3P_FAMILY_GAUSS_MEAN, d, False), b_col=-1) == UNSUPPORTED
    assert call(_struct(poi, d, True, guide=L.D3P_GUIDE_EXP_SITES)) == UNSUPPORTED
    assert b"D3P_GUIDE_EXP_SITES" in L.load().d3p_last_error()
    for sigma in (0.0, -1.0, float("inf"), float("nan")):
        assert call(_struct(lin, d, True, sigma=sigma)) == INVALID
    assert call(None) == INVALID
    assert call(_struct(poi, d, True), X_=None) == INVALID and call(_struct(poi, d, True), obs_=None) == INVALID
    assert call(_struct(poi, d, True), okeys_=None) == INVALID and call(_struct(poi, d, True), lat_=None) == INVALID
    assert call(_struct(poi, d, True), n_=0) == INVALID and call(_struct(poi, d, True), d_=d + 1) == INVALID
    assert call(_struct(poi, d, True), b_col=-1) == INVALID and call(_struct(poi, d, False)) == INVALID
    assert call(_struct(poi, d, True), b_col=1) == INVALID and call(_struct(poi, d, True), ld=d) == INVALID and call(_struct(poi, d, True), w_off=2) == INVALID
    assert call(_struct(poi, d, True), rows_=2 ** 31) == INVALID        # 2 rows < 2^32 (Poisson)
    assert call(_struct(lin, d, True), rows_=2 ** 32) == INVALID
    assert call(_struct(poi, d, True), X_=torch.zeros(rows, d)) == INVALID          # host memory
    assert call(_struct(poi, d, True), rows_=0) == 0 and call(_struct(lin, d, True), rows_=0) == 0
    torch.cuda.synchronize()
    assert bool((obs == 77).all())
    assert call(_struct(poi, d, True)) == 0
    torch.cuda.synchronize()
    assert bool((obs != 77).all())          # t = 0: Poisson(1) draws, at most a handful
