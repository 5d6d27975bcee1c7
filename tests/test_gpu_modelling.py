"""Predictive sampling (d3p_amd.modelling) on the GPU against the oracle's threefry primitives (the reference's
tests/test_modelling.py:31-250 re-expressed, plus bit-level checks of the key plumbing stated in DESIGN.md section 4b).

The CPU restatement of section 4b and the tolerances of every check live in tests/predictive_ref.py (its docstring states them).
"""
import math

import numpy as np
import pytest
import torch

from d3p_amd import modelling as M
from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, GaussianMean, LogisticRegression, MeanFieldGuide,
                            VAEGuide, VAEModel)

from .predictive_ref import (assert_bernoulli as _assert_bernoulli, assert_latent as _assert_latent, chains as _chains,
                             check_logreg as _check_logreg, dense_bound as _dense_bound, key as _key, logreg_expect as _logreg_expect,
                             logreg_params as _logreg_params, np_ as _np, site_key as _site_key, vae_decode_bound as _vae_decode_bound,
                             vae_net as _vae_net)

pytestmark = pytest.mark.gpu


LOGREG_CASES = [(False, AutoDiagonalNormal), (True, AutoDiagonalNormal), (False, DiagonalNormalGuide), (True, DiagonalNormalGuide),
                (True, MeanFieldGuide)]


# ------------------------------------------------------------------------------- 1. small shapes against the oracle
@pytest.mark.parametrize("intercept,G", LOGREG_CASES)
@pytest.mark.parametrize("multi", [False, True])
def test_logreg_posterior_against_oracle(gpu, O, intercept, G, multi):
    rng = np.random.default_rng(1 + intercept + 2 * multi)
    d, rows, n = 5, 77, 9
    model = LogisticRegression(d, intercept=intercept)
    guide = G(model)
    params = _logreg_params(guide, d, intercept, rng)
    X = rng.normal(size=(rows, d)).astype(np.float32)
    key = _key(17)
    if multi:
        res = M.sample_multi_posterior_predictive(key, n, model, (torch.tensor(X).cuda(),), guide, (X,), params)
    else:
        res = M.sample_posterior_predictive(key, model, (X,), guide, (X,), params)
    nn = n if multi else 1
    exp, okeys = _logreg_expect(O, _np(key), nn, multi, model, guide, params, X)
    expected_sites = {"w", "obs"} | ({"intercept"} if intercept else set()) | ({"_auto_latent"} if G is AutoDiagonalNormal else set())
    assert expected_sites <= set(res)
    assert res["obs"].dtype == torch.int32 and tuple(res["obs"].shape) == ((n, rows) if multi else (rows,))
    _check_logreg(O, res, exp, okeys, X, d, intercept, nn, f"{G.__name__} intercept={intercept}")


@pytest.mark.parametrize("subst", [None, ("w",), ("intercept",), ("w", "intercept")])
def test_logreg_prior_against_oracle(gpu, O, subst):
    rng = np.random.default_rng(5)
    d, rows, n = 4, 100, 6
    model = LogisticRegression(d, prior_scale=2.0, intercept=True, intercept_prior_scale=0.5)
    X = rng.normal(size=(rows, d)).astype(np.float32)
    values = {"w": rng.normal(size=d).astype(np.float32), "intercept": np.float32(0.3)}
    sub = {k: values[k] for k in (subst or ())}
    key = _key(3)
    res = M.sample_multi_prior_predictive(key, n, model, (X,), sub)
    exp, okeys = _logreg_expect(O, _np(key), n, True, model, None, None, X, sub)
    _check_logreg(O, res, exp, okeys, X, d, True, n, f"prior subst={subst}")
    one = M.sample_prior_predictive(key, model, (X,), sub)
    exp1, okeys1 = _logreg_expect(O, _np(key), 1, False, model, None, None, X, sub)
    _check_logreg(O, {k: v.unsqueeze(0) for k, v in one.items()}, exp1, okeys1, X, d, True, 1, f"single prior subst={subst}")


@pytest.mark.parametrize("G", [AutoDiagonalNormal, DiagonalNormalGuide, None])
def test_gaussian_mean_against_oracle(gpu, O, G):
    rng = np.random.default_rng(11)
    d, rows, n = 3, 41, 5
    model = GaussianMean(d, prior_scale=1.0, obs_scale=0.1)
    key = _key(23)
    if G is None:
        res = M.sample_multi_prior_predictive(key, n, model, (None, rows, d))
        params = None
    else:
        guide = G(model)
        params = ({"auto_loc": rng.normal(size=d).astype(np.float32), "auto_scale": rng.uniform(0.1, 0.3, d).astype(np.float32)}
                  if G is AutoDiagonalNormal else
                  {"mu_loc": rng.normal(size=d).astype(np.float32), "mu_std_log": rng.uniform(-2, -1, d).astype(np.float32)})
        res = M.sample_multi_posterior_predictive(key, n, model, (None, rows), guide, (None, rows), params)
    assert tuple(res["obs"].shape) == (n, rows, d) and tuple(res["mu"].shape) == (n, d)
    for i, dk in enumerate(O.tf_split(_np(key), n)):
        mk, gk = _chains(O, dk, G is not None)
        if G is None:
            eps = O.tf_normal(_site_key(O, mk, 0), d)
            _assert_latent(_np(res["mu"][i]), np.zeros(d, np.float32), eps, np.ones(d), "prior mu")
            okey = _site_key(O, mk, 1)
        else:
            eps = O.tf_normal(_site_key(O, gk, 0), d)
            loc, sc = ((params["auto_loc"], params["auto_scale"].astype(np.float64)) if G is AutoDiagonalNormal else
                       (params["mu_loc"], np.exp(params["mu_std_log"].astype(np.float64))))
            _assert_latent(_np(res["mu"][i]), loc, eps, sc, "posterior mu")
            okey = _site_key(O, mk, 0)
        mu = _np(res["mu"][i])
        eps_o = O.tf_normal(okey, rows * d).reshape(rows, d)
        _assert_latent(_np(res["obs"][i]), np.broadcast_to(mu, (rows, d)), eps_o, np.full((rows, d), 0.1, np.float32), "obs")


def test_gaussian_mean_substituted_mu_is_returned_as_given(gpu, O):
    d, rows = 4, 10
    mu = np.arange(d, dtype=np.float32)
    res = M.sample_prior_predictive(_key(2), GaussianMean(d), (None, rows, d), {"mu": mu})
    assert np.array_equal(_np(res["mu"]), mu)
    eps = O.tf_normal(_site_key(O, _np(_key(2)), 0), rows * d).reshape(rows, d)    # mu took no key: obs is the handler's first
    _assert_latent(_np(res["obs"]), np.broadcast_to(mu, (rows, d)), eps, np.full((rows, d), 0.1, np.float32), "obs")


# ------------------------------------------------------------------------------- VAE
@pytest.mark.parametrize("H,H2", [(40, 0), (40, 24)])
@pytest.mark.parametrize("posterior", [True, False])
def test_vae_against_oracle(gpu, O, H, H2, posterior):
    rng = np.random.default_rng(H + H2 + posterior)
    D, Z, B, n = 60, 7, 5, 4
    tree, ldec, lenc, (Wl, bl, Ws, bs) = _vae_net(D, H, Z, H2, rng)
    model = VAEModel(Z, (H, H2) if H2 else H)
    X = (rng.random((B, D)) < 0.3).astype(np.float32)
    key = _key(31)
    if posterior:
        res = M.sample_multi_posterior_predictive(key, n, model, (B, Z, model.hidden_dim, D), VAEGuide(model), (X, Z, H), tree)
    else:
        res = M.sample_multi_prior_predictive(key, n, model, (B, Z, model.hidden_dim, D), {"decoder$params": tree["decoder$params"]})
    assert tuple(res["z"].shape) == (n, B, Z) and tuple(res["obs"].shape) == (n, B, D) and res["obs"].dtype == torch.int32
    z_dev = _np(res["z"])
    if posterior:
        h, E = X.astype(np.float64), np.zeros(X.shape)
        for W, b in lenc:
            h, E = _dense_bound(h, E, W, b, True)
        zl, El = _dense_bound(h, E, Wl, bl, False)
        zs, Es = _dense_bound(h, E, Ws, bs, False)
    for i, dk in enumerate(O.tf_split(_np(key), n)):
        mk, gk = _chains(O, dk, posterior)
        eps = O.tf_normal(_site_key(O, gk if posterior else mk, 0), B * Z).reshape(B, Z).astype(np.float64)
        if posterior:
            ref = zl + eps * np.exp(zs)
            tol = (El + np.abs(eps) * np.exp(zs) * (np.expm1(Es) + 2.0 ** -22) + 2.0 ** -22 * (np.abs(zl) + np.abs(eps) * np.exp(zs))
                   + (2e-6 * np.abs(eps) + 2e-7) * np.exp(zs) + 1e-30)
            okey = _site_key(O, mk, 0)
        else:
            ref, tol = eps, 2e-6 * np.abs(eps) + 2e-7    # z = 0 + eps * 1 exactly: the normal() tolerance alone
            okey = _site_key(O, mk, 1)
        err = np.abs(z_dev[i] - ref)
        assert np.all(err <= tol), f"z[{i}]: max err {err.max()}"
        logits, Eo = _vae_decode_bound(z_dev[i], ldec)
        band = Eo / 4 + 2.0 ** -21
        _assert_bernoulli(_np(res["obs"][i]).ravel(), O.tf_uniform(okey, B * D), (1 / (1 + np.exp(-logits))).ravel(), band.ravel(),
                          f"vae obs[{i}]")


def test_vae_prior_with_z_substituted(gpu, O):
    rng = np.random.default_rng(9)
    D, Z, H, B = 30, 5, 16, 3
    tree, ldec, _, _ = _vae_net(D, H, Z, 0, rng, scale=0.3)
    zval = rng.normal(size=(B, Z)).astype(np.float32)
    key = _key(8)
    res = M.sample_multi_prior_predictive(key, 3, VAEModel(Z, H), (B, Z, H, D), {"decoder$params": tree["decoder$params"], "z": zval})
    assert np.array_equal(_np(res["z"]), np.broadcast_to(zval, (3, B, Z)))
    logits, Eo = _vae_decode_bound(zval, ldec)
    for i, dk in enumerate(O.tf_split(_np(key), 3)):
        _assert_bernoulli(_np(res["obs"][i]).ravel(), O.tf_uniform(_site_key(O, dk, 0), B * D), (1 / (1 + np.exp(-logits))).ravel(),
                          (Eo / 4 + 2.0 ** -21).ravel(), "obs")


# ------------------------------------------------------------------------------- 2. the vmap identity
@pytest.mark.parametrize("n", [1, 37, 128, 129])
@pytest.mark.parametrize("rows", [1, 63, 100003])
def test_multi_draw_i_is_the_single_draw_of_split_key_i(gpu, n, rows):
    import d3p_amd.random.debug as jr
    rng = np.random.default_rng(n + rows)
    d = 6
    model = LogisticRegression(d, intercept=True)
    guide = AutoDiagonalNormal(model)
    params = _logreg_params(guide, d, True, rng)
    X = torch.tensor(rng.normal(size=(rows, d)).astype(np.float32)).cuda()
    key = _key(n * 7 + rows)
    multi = M.sample_multi_posterior_predictive(key, n, model, (X,), guide, (X,), params)
    again = M.sample_multi_posterior_predictive(key, n, model, (X,), guide, (X,), params)
    for k in multi:
        assert torch.equal(multi[k], again[k]), k
    keys = jr.split(key, n)
    for i in sorted({0, n // 2, n - 1}):
        one = M.sample_posterior_predictive(keys[i].contiguous(), model, (X,), guide, (X,), params)
        for k in one:
            assert torch.equal(multi[k][i], one[k]), (k, i)


# ------------------------------------------------------------------------------- 3. production shape
@pytest.mark.parametrize("G", [AutoDiagonalNormal, DiagonalNormalGuide, MeanFieldGuide])
def test_logreg_production_shape(gpu, G):
    import d3p_amd.random.debug as jr
    d, rows, n = 512, 1_000_000, 128
    rng = np.random.default_rng(7)
    model = LogisticRegression(d, intercept=True)
    guide = G(model)
    params = _logreg_params(guide, d, True, rng)
    for k in params:
        params[k] = params[k] * np.float32(0.1) if k.endswith("_loc") else params[k]
    X = torch.randn((rows, d), device="cuda")
    key = _key(99)
    res = M.sample_multi_posterior_predictive(key, n, model, (X,), guide, (X,), params)
    obs = res["obs"]
    assert tuple(obs.shape) == (n, rows) and obs.dtype == torch.int32
    w = res["w"].double()
    b = res["intercept"].double().reshape(n)
    plan = M.site_plan(model, guide, d=d, rows=rows)
    okey_index = next(s.key_index for s in plan if s.name == "obs")
    draw_keys = jr.split(key, n)
    Xd = X.double()
    Xa = Xd.abs()
    gamma = (d + 2) * 2.0 ** -23
    for i in [0, 1, 63, 64, 127]:
        mk = jr.split(draw_keys[i].contiguous(), 2)[0].contiguous()
        c = mk
        for _ in range(okey_index + 1):
            kk = jr.split(c, 2)
            c, s = kk[0].contiguous(), kk[1].contiguous()
        u = jr.uniform(s, (rows,)).double()
        logit = Xd @ w[i] + b[i]
        p = torch.sigmoid(logit)
        band = gamma * (Xa @ w[i].abs() + b[i].abs()) / 4 + 2.0 ** -21
        exp = (u < p).to(torch.int32)
        bad = (obs[i] != exp) & ((u - p).abs() > band)
        assert int(bad.sum()) == 0, f"draw {i}: {int(bad.sum())} outcomes outside the band"
    # the outcomes are Bernoulli(p): the mean over all draws agrees with the mean probability
    assert abs(float(obs.double().mean()) - float(torch.sigmoid(Xd[:4096] @ w.T + b).mean())) < 0.02


@pytest.mark.parametrize("H,H2", [(400, 0), (400, 200)])
def test_vae_production_shape(gpu, O, H, H2):
    rng = np.random.default_rng(H2 + 1)
    D, Z, B, n = 784, 50, 128, 10
    tree, ldec, lenc, (Wl, bl, Ws, bs) = _vae_net(D, H, Z, H2, rng, scale=0.05)
    model = VAEModel(Z, (H, H2) if H2 else H)
    X = (rng.random((B, D)) < 0.2).astype(np.float32)
    key = _key(5)
    res = M.sample_multi_posterior_predictive(key, n, model, (B, Z, model.hidden_dim, D), VAEGuide(model), (X, Z, H), tree)
    z_dev, obs = _np(res["z"]), _np(res["obs"])
    for i, dk in enumerate(O.tf_split(_np(key), n)[:3]):
        mk, _ = _chains(O, dk, True)
        logits, Eo = _vae_decode_bound(z_dev[i], ldec)
        _assert_bernoulli(obs[i].ravel(), O.tf_uniform(_site_key(O, mk, 0), B * D), (1 / (1 + np.exp(-logits))).ravel(),
                          (Eo / 4 + 2.0 ** -21).ravel(), f"vae obs[{i}]")


# ------------------------------------------------------------------------------- 4. the reference's own cases (tests/test_modelling.py)
def _gm():
    return GaussianMean(3, prior_scale=1.0, obs_scale=0.1)


@pytest.mark.parametrize("with_intermediates", [False, True])
def test_reference_prior_shapes_and_structure(gpu, with_intermediates):
    rows, n = 100, 20
    r1 = M.sample_prior_predictive(_key(0), _gm(), (None, rows, 3), with_intermediates=with_intermediates)
    rn = M.sample_multi_prior_predictive(_key(0), n, _gm(), (None, rows, 3), with_intermediates=with_intermediates)
    assert set(r1) == {"mu", "obs"} and set(rn) == {"mu", "obs"}
    if with_intermediates:
        for r in (r1, rn):
            for v in r.values():
                assert isinstance(v, tuple) and len(v) == 2 and v[1] == []
        r1 = {k: v[0] for k, v in r1.items()}
        rn = {k: v[0] for k, v in rn.items()}
    assert tuple(r1["mu"].shape) == (3,) and tuple(r1["obs"].shape) == (rows, 3)
    assert tuple(rn["mu"].shape) == (n, 3) and tuple(rn["obs"].shape) == (n, rows, 3)


def test_reference_prior_substitute_and_moments(gpu):
    rows = 10000
    mu = torch.tensor([1.0, -2.0, 0.5], device="cuda")
    r = M.sample_prior_predictive(_key(1), _gm(), (None, rows, 3), {"mu": mu})
    assert torch.equal(r["mu"], mu)
    obs = r["obs"].double()
    # crude 3 sigma checks: mean of rows ~ mu (se 0.1 / sqrt(N)), std ~ 0.1 (se ~ 0.1 / sqrt(2N))
    assert torch.all((obs.mean(0) - mu.double()).abs() < 3 * 0.1 / math.sqrt(rows))
    assert torch.all((obs.std(0) - 0.1).abs() < 3 * 0.1 / math.sqrt(2 * rows))
    rn = M.sample_multi_prior_predictive(_key(2), 2000, _gm(), (None, 1, 3))
    m = rn["mu"].double()
    assert torch.all(m.mean(0).abs() < 3 / math.sqrt(2000)) and torch.all((m.std(0) - 1).abs() < 3 / math.sqrt(2 * 2000))


@pytest.mark.parametrize("with_intermediates", [False, True])
def test_reference_posterior_shapes_and_moments(gpu, with_intermediates):
    rows, n = 50, 3000
    model = _gm()
    guide = DiagonalNormalGuide(model)
    loc = np.array([0.5, -1.0, 2.0], np.float32)
    params = {"mu_loc": loc, "mu_std_log": np.log(np.full(3, 0.2, np.float32))}
    r1 = M.sample_posterior_predictive(_key(4), model, (None, rows), guide, (None, rows), params, with_intermediates=with_intermediates)
    rn = M.sample_multi_posterior_predictive(_key(4), n, model, (None, rows), guide, (None, rows), params,
                                             with_intermediates=with_intermediates)
    if with_intermediates:
        assert all(isinstance(v, tuple) and v[1] == [] for v in list(r1.values()) + list(rn.values()))
        r1 = {k: v[0] for k, v in r1.items()}
        rn = {k: v[0] for k, v in rn.items()}
    assert set(r1) == {"mu", "obs"} and tuple(r1["obs"].shape) == (rows, 3) and tuple(rn["obs"].shape) == (n, rows, 3)
    m = rn["mu"].double()
    assert torch.all((m.mean(0) - torch.tensor(loc, dtype=torch.float64, device="cuda")).abs() < 3 * 0.2 / math.sqrt(n))
    assert torch.all((m.std(0) - 0.2).abs() < 3 * 0.2 / math.sqrt(2 * n))
    resid = rn["obs"].double() - m[:, None, :]
    assert abs(float(resid.std()) - 0.1) < 3 * 0.1 / math.sqrt(2 * resid.numel())


# ------------------------------------------------------------------------------- 5. end to end
def test_logistic_regression_posterior_predictive_accuracy(gpu):
    import importlib.util
    import os
    import d3p_amd.random as rng_suite
    import d3p_amd.random.debug as jr
    from d3p_amd.minibatch import poisson_batchify_data
    from d3p_amd.models import Adam, Trace_ELBO
    from d3p_amd.svi import DPSVI
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ex_logreg_pp", os.path.join(root, "examples", "logistic_regression.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    N, d, batch = 10000, 4, 200
    train, test = mod.create_toy_data(N, d)
    model = LogisticRegression(d, prior_scale=1.0, intercept=True)
    guide = AutoDiagonalNormal(model)
    train_init, train_fetch = poisson_batchify_data(train, batch / N, max_batch_size=.99, rng_suite=rng_suite)
    key = rng_suite.PRNGKey(0)
    key, init_key, fetch_key = rng_suite.split(key, 3)
    _, bstate = train_init(rng_key=fetch_key)
    svi = DPSVI(model, guide, Adam(5e-2), Trace_ELBO(), dp_scale=0.5, clipping_threshold=1., num_obs_total=N, rng_suite=rng_suite)
    state = svi.init(init_key, *train_fetch(0, bstate)[0])
    for _ in range(8):
        key, fetch_key = rng_suite.split(key, 2)
        nb, bstate = train_init(rng_key=fetch_key)
        state, _ = svi.run_steps(state, train_fetch, bstate, 0, nb)
    acc = mod.estimate_accuracy(test[0], test[1], model, guide, svi.get_params(state), jr.PRNGKey(1), 100)
    assert acc > 0.7, acc
