"""Predictive sampling at the places where its kernels branch, every draw checked against the oracle (tests/predictive_ref.py states
the CPU restatement and every tolerance used here).

k_predict_logreg works on tiles of 128 draws x 128 rows and stages K in slices of 32, the next slice prefetched into registers: the
cases below put d on both sides of a slice (1, 31, 32, 33, 63, 65, 100, 257, 513), the rows on both sides of a row tile and the draws
in a second and third draw tile, each rows and n value together with a d above 32 that is not a multiple of 32 (a partial last slice
that was prefetched).  With dyadic inputs every logit is exact in float32, so the band shrinks to the sigmoid's 2^-21 and a dropped
or duplicated K column, row or intercept is caught outright.  The two-rounding rule of normal_site_value is checked bit for bit.
The VAE's z is checked where the encoder runs on the bf16x3 product (B > 96), the decoder alone on it (n B > 96, B <= 96), at
Z % 4 != 0 and at an odd B D (the padded last threefry counter pair of k_predict_vae_obs)."""
import numpy as np
import pytest
import torch

from d3p_amd import modelling as M
from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, GaussianMean, LogisticRegression, MeanFieldGuide, VAEGuide,
                            VAEModel)

from .predictive_ref import (assert_bernoulli, assert_latent, assert_not_vacuous, chains, check_logreg, check_vae_obs, key,
                             logreg_expect, logreg_params, np_, site_key, vae_encode_bound, vae_net, vae_posterior_z_ref)

pytestmark = pytest.mark.gpu

GUIDES = {"auto": AutoDiagonalNormal, "diag": DiagonalNormalGuide, "meanfield": MeanFieldGuide}


def _multi(n):
    return n is not None


def _run_logreg(k, n, model, X, guide=None, params=None, subst=None):
    if guide is None:
        if n is None:
            return M.sample_prior_predictive(k, model, (X,), subst)
        return M.sample_multi_prior_predictive(k, n, model, (X,), subst)
    if n is None:
        return M.sample_posterior_predictive(k, model, (X,), guide, (X,), params)
    return M.sample_multi_posterior_predictive(k, n, model, (X,), guide, (X,), params)


def _lead(res, n):
    """The single form's sites with the leading draw axis of the multi form."""
    return res if n is not None else {k: v.unsqueeze(0) for k, v in res.items()}


# ------------------------------------------------------------------------------- logistic regression: tile edges
# (d, rows, n, what): what = a guide of GUIDES (with an intercept unless it ends in '-'), or 'prior:' + the substituted sites
LOGREG_EDGES = [
    (1, 129, None, "auto"),
    (31, 255, 129, "diag"),
    (32, 128, 128, "meanfield"),
    (33, 1, 257, "auto"),
    (63, 2, 127, "meanfield"),
    (65, 3, 129, "prior:"),
    (100, 127, 1, "prior:w"),
    (257, 257, None, "prior:intercept"),
    (513, 4097, 129, "auto"),
    (33, 128, 257, "diag"),
    (100, 4097, 128, "prior:w,intercept"),
    (65, 255, None, "diag-"),
    (513, 129, 1, "meanfield"),
    (257, 1, 127, "auto-"),
]


@pytest.mark.parametrize("d,rows,n,what", LOGREG_EDGES)
def test_logreg_tile_edges_every_draw(gpu, O, d, rows, n, what):
    rng = np.random.default_rng(d * 10007 + rows * 13 + (n or 0))
    X = rng.normal(size=(rows, d)).astype(np.float32)
    k = key(d + 7 * rows + 131 * (n or 0))
    nn = n or 1
    if what.startswith("prior:"):
        model = LogisticRegression(d, prior_scale=0.3, intercept=True, intercept_prior_scale=1.5)
        values = {"w": (0.3 * rng.normal(size=d)).astype(np.float32), "intercept": np.float32(-0.7)}
        sub = {s: values[s] for s in what[6:].split(",") if s}
        res = _run_logreg(k, n, model, X, subst=sub)
        exp, okeys = logreg_expect(O, np_(k), nn, _multi(n), model, None, None, X, sub)
        intercept = True
    else:
        intercept = not what.endswith("-")
        model = LogisticRegression(d, intercept=intercept)
        guide = GUIDES[what.rstrip("-")](model)
        params = logreg_params(guide, d, intercept, rng)
        for p in params:        # logits of a few units: outcomes that are neither all 0 nor all 1
            if p.endswith("_loc"):
                params[p] = (params[p] * np.float32(2.0 / np.sqrt(d))).astype(np.float32)
        res = _run_logreg(k, n, model, X, guide, params)
        exp, okeys = logreg_expect(O, np_(k), nn, _multi(n), model, guide, params, X)
    assert tuple(res["obs"].shape) == ((n, rows) if n is not None else (rows,)) and res["obs"].dtype == torch.int32
    share = check_logreg(O, _lead(res, n), exp, okeys, X, d, intercept, nn, f"d={d} rows={rows} n={n} {what}", sharp=True)
    assert_not_vacuous(share, nn * rows)


# ------------------------------------------------------------------------------- exact logits (dyadic inputs)
@pytest.mark.parametrize("d,rows,n", [(33, 129, 257), (65, 4097, 129), (513, 257, None), (100, 3, 128), (257, 255, 127), (63, 1, 129)])
def test_logreg_exact_logits(gpu, O, d, rows, n):
    """X in {0, +-1/2, +-1}, w = m / 64 with m in +-[1, 8], b = m / 128: every product is a multiple of 2^-7 and every partial sum
    stays below 2^17 of them, so the float32 logit is exact in any order and only the sigmoid's 2^-21 is left of the band."""
    rng = np.random.default_rng(d + rows + (n or 0))
    X = (rng.integers(-2, 3, size=(rows, d)) / 2).astype(np.float32)
    w = (rng.integers(1, 9, size=d) * rng.choice([-1, 1], size=d) / 64).astype(np.float32)
    b = np.float32(rng.integers(-40, 41) / 128)
    model = LogisticRegression(d, intercept=True)
    k = key(1000 + d)
    res = _run_logreg(k, n, model, X, subst={"w": w, "intercept": b})
    nn = n or 1
    obs = np_(res["obs"]).reshape(nn, rows)
    logit = X.astype(np.float64) @ w.astype(np.float64) + float(b)
    p = 1 / (1 + np.exp(-logit))
    shares = [assert_bernoulli(obs[i], O.tf_uniform(site_key(O, dk, 0), rows), p, np.full(rows, 2.0 ** -21), f"draw {i}")
              for i, dk in enumerate(O.tf_split(np_(k), nn) if n is not None else [np_(k)])]
    assert_not_vacuous(float(np.mean(shares)), nn * rows)


# ------------------------------------------------------------------------------- the two-rounding rule, bit for bit
def _f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("kind", ["logreg_auto", "logreg_prior", "gauss_auto", "gauss_obs"])
def test_normal_site_value_rounds_twice(gpu, kind):
    """normal_site_value = fl(loc + fl(eps scale)): the device's eps is read through a call with loc = 0 and scale = 1 (exact), then the
    same key plan with random float32 loc and scale must give np.float32(loc) + np.float32(eps) * np.float32(scale) bit for bit; a
    fused multiply-add differs in the last bit in a good share of the elements."""
    rng = np.random.default_rng(41)
    k, n = key(77), 129
    if kind.startswith("logreg"):
        d, rows = 100, 3
        X = rng.normal(size=(rows, d)).astype(np.float32)
        if kind == "logreg_auto":
            model = LogisticRegression(d, intercept=True)
            guide = AutoDiagonalNormal(model)
            eps = np_(M.sample_multi_posterior_predictive(k, n, model, (X,), guide, (X,), {"auto_loc": np.zeros(d + 1, np.float32),
                                                                                             "auto_scale": np.ones(d + 1, np.float32)})["_auto_latent"])
            loc = (3 * rng.normal(size=d + 1)).astype(np.float32)
            scale = rng.uniform(0.01, 3.0, d + 1).astype(np.float32)
            got = np_(M.sample_multi_posterior_predictive(k, n, model, (X,), guide, (X,), {"auto_loc": loc, "auto_scale": scale})["_auto_latent"])
        else:
            one = M.sample_multi_prior_predictive(k, n, LogisticRegression(d, prior_scale=1.0, intercept=True, intercept_prior_scale=1.0), (X,))
            eps = np.concatenate([np_(one["w"]), np_(one["intercept"]).reshape(n, 1)], axis=1)
            s_w, s_b = np.float32(rng.uniform(0.1, 5)), np.float32(rng.uniform(0.1, 5))
            two = M.sample_multi_prior_predictive(k, n, LogisticRegression(d, prior_scale=float(s_w), intercept=True,
                                                                           intercept_prior_scale=float(s_b)), (X,))
            got = np.concatenate([np_(two["w"]), np_(two["intercept"]).reshape(n, 1)], axis=1)
            loc = np.zeros(d + 1, np.float32)
            scale = np.array([s_w] * d + [s_b], np.float32)
    elif kind == "gauss_auto":
        d, rows = 33, 5
        model = GaussianMean(d)
        guide = AutoDiagonalNormal(model)
        eps = np_(M.sample_multi_posterior_predictive(k, n, model, (None, rows), guide, (None, rows),
                                                      {"auto_loc": np.zeros(d, np.float32), "auto_scale": np.ones(d, np.float32)})["mu"])
        loc = (3 * rng.normal(size=d)).astype(np.float32)
        scale = rng.uniform(0.01, 3.0, d).astype(np.float32)
        got = np_(M.sample_multi_posterior_predictive(k, n, model, (None, rows), guide, (None, rows), {"auto_loc": loc, "auto_scale": scale})["mu"])
    else:
        d, rows = 33, 41     # rows d odd: the last threefry counter pair is padded
        eps = np_(M.sample_multi_prior_predictive(k, n, GaussianMean(d, obs_scale=1.0), (None, rows, d), {"mu": np.zeros(d, np.float32)})["obs"])
        mu = (3 * rng.normal(size=d)).astype(np.float32)
        s = np.float32(0.37)
        got = np_(M.sample_multi_prior_predictive(k, n, GaussianMean(d, obs_scale=float(s)), (None, rows, d), {"mu": mu})["obs"])
        loc, scale = np.broadcast_to(mu, (rows, d)), np.full((rows, d), s, np.float32)
    want = loc + eps * scale        # float32 numpy: a product rounded to float32, then a sum rounded to float32
    assert want.dtype == np.float32
    bad = _f32_bits(got) != _f32_bits(want)
    assert not bad.any(), f"{kind}: {int(bad.sum())} of {bad.size} values are not fl(loc + fl(eps scale)) (first at {np.argwhere(bad)[0]})"


# ------------------------------------------------------------------------------- VAE
# (posterior, B, D, H, H2, Z, n, z substituted)
VAE_EDGES = [
    (True, 97, 60, 40, 0, 8, 3, False),     # encoder on bf16x3 (B > 96), Z % 4 = 0: every head product 16-byte
    (True, 128, 64, 40, 24, 4, 2, False),
    (True, 200, 60, 40, 24, 7, 2, False),   # Z % 4 != 0: the heads and the first decoder product on the scalar-fetch path
    (True, 7, 60, 40, 0, 8, 16, False),     # n B = 112 rows: the decoder on bf16x3, the encoder (7 rows) not
    (True, 7, 33, 16, 0, 7, 5, False),      # B D = 231 odd: the padded last counter pair of k_predict_vae_obs
    (False, 7, 33, 24, 24, 4, 16, False),
    (False, 97, 60, 40, 0, 7, 2, False),
    (False, 7, 60, 40, 0, 8, 16, True),
    (False, 5, 33, 16, 24, 7, 3, True),
]


@pytest.mark.parametrize("posterior,B,D,H,H2,Z,n,zsub", VAE_EDGES)
def test_vae_edges_every_draw(gpu, O, posterior, B, D, H, H2, Z, n, zsub):
    rng = np.random.default_rng(B * 1009 + D + Z + H2)
    tree, ldec, lenc, heads = vae_net(D, H, Z, H2, rng, scale=0.15)
    model = VAEModel(Z, (H, H2) if H2 else H)
    k = key(B + 3 * D)
    zval = rng.normal(size=(B, Z)).astype(np.float32)
    if posterior:
        X = (rng.random((B, D)) < 0.3).astype(np.float32)
        res = M.sample_multi_posterior_predictive(k, n, model, (B, Z, model.hidden_dim, D), VAEGuide(model), (X, Z, H), tree)
        zl, El, zs, Es = vae_encode_bound(X, lenc, heads)
    else:
        sub = {"decoder$params": tree["decoder$params"], **({"z": zval} if zsub else {})}
        res = M.sample_multi_prior_predictive(k, n, model, (B, Z, model.hidden_dim, D), sub)
    assert tuple(res["z"].shape) == (n, B, Z) and tuple(res["obs"].shape) == (n, B, D) and res["obs"].dtype == torch.int32
    z_dev, obs = np_(res["z"]), np_(res["obs"])
    shares = []
    for i, dk in enumerate(O.tf_split(np_(k), n)):
        mk, gk = chains(O, dk, posterior)
        if zsub:
            assert np.array_equal(z_dev[i], zval), f"z[{i}] is not the substituted value"
            okey = site_key(O, mk, 0)
        else:
            eps = O.tf_normal(site_key(O, gk if posterior else mk, 0), B * Z).reshape(B, Z).astype(np.float64)
            ref, tol = vae_posterior_z_ref(zl, El, zs, Es, eps) if posterior else (eps, 2e-6 * np.abs(eps) + 2e-7)
            err = np.abs(z_dev[i] - ref)
            assert np.all(err <= tol), f"z[{i}]: max err {err.max()} (tol at argmax {tol.ravel()[err.argmax()]})"
            okey = site_key(O, mk, 0 if posterior else 1)
        shares.append(check_vae_obs(O, obs[i], z_dev[i], ldec, okey, f"vae obs[{i}]"))
    assert_not_vacuous(float(np.mean(shares)), n * B * D)


# ------------------------------------------------------------------------------- Gaussian mean
# (guide or None for the prior with mu substituted, d, rows, n)
GAUSS_EDGES = [
    ("auto", 33, 41, 129),      # rows d odd
    ("diag", 257, 3, None),     # odd
    (None, 1, 129, 129),        # odd
    ("auto", 1, 2, None),       # even
    ("diag", 33, 64, 129),      # even
    (None, 257, 4, None),       # even
]


@pytest.mark.parametrize("G,d,rows,n", GAUSS_EDGES)
def test_gaussian_mean_edges_every_draw(gpu, O, G, d, rows, n):
    rng = np.random.default_rng(d * 31 + rows)
    model = GaussianMean(d, prior_scale=1.0, obs_scale=0.25)
    k = key(d + rows)
    nn = n or 1
    if G is None:
        mu_sub = rng.normal(size=d).astype(np.float32)
        if n is not None:
            res = M.sample_multi_prior_predictive(k, n, model, (None, rows, d), {"mu": mu_sub})
        else:
            res = M.sample_prior_predictive(k, model, (None, rows, d), {"mu": mu_sub})
    else:
        guide = {"auto": AutoDiagonalNormal, "diag": DiagonalNormalGuide}[G](model)
        params = ({"auto_loc": rng.normal(size=d).astype(np.float32), "auto_scale": rng.uniform(0.1, 0.3, d).astype(np.float32)}
                  if G == "auto" else
                  {"mu_loc": rng.normal(size=d).astype(np.float32), "mu_std_log": rng.uniform(-2, -1, d).astype(np.float32)})
        if n is not None:
            res = M.sample_multi_posterior_predictive(k, n, model, (None, rows), guide, (None, rows), params)
        else:
            res = M.sample_posterior_predictive(k, model, (None, rows), guide, (None, rows), params)
    res = _lead(res, n)
    assert tuple(res["obs"].shape) == (nn, rows, d)
    dks = O.tf_split(np_(k), nn) if n is not None else [np_(k)]
    for i, dk in enumerate(dks):
        mk, gk = chains(O, dk, G is not None)
        mu = np_(res["mu"]).reshape(nn, d)[i]
        if G is None:
            assert np.array_equal(mu, mu_sub)
            okey = site_key(O, mk, 0)
        else:
            eps = O.tf_normal(site_key(O, gk, 0), d)
            loc, sc = ((params["auto_loc"], params["auto_scale"].astype(np.float64)) if G == "auto" else
                       (params["mu_loc"], np.exp(params["mu_std_log"].astype(np.float64))))
            assert_latent(mu, loc, eps, sc, f"posterior mu[{i}]")
            okey = site_key(O, mk, 0)
        eps_o = O.tf_normal(okey, rows * d).reshape(rows, d)
        assert_latent(np_(res["obs"][i]), np.broadcast_to(mu, (rows, d)), eps_o, np.full((rows, d), 0.25, np.float32), f"obs[{i}]")


# ------------------------------------------------------------------------------- input forms and streams
@pytest.mark.parametrize("form", ["numpy_f64", "strided_view", "int32_key", "side_stream"])
@pytest.mark.parametrize("n", [None, 129])
def test_input_forms_are_bitwise_the_contiguous_call(gpu, form, n):
    rng = np.random.default_rng(3)
    d, rows = 33, 257
    model = LogisticRegression(d, intercept=True)
    guide = AutoDiagonalNormal(model)
    params = logreg_params(guide, d, True, rng)
    X = rng.normal(size=(rows, d)).astype(np.float32)
    Xt = torch.tensor(X, device="cuda")
    k = key(5)
    base = _run_logreg(k, n, model, Xt, guide, params)
    torch.cuda.synchronize()
    if form == "numpy_f64":
        got = _run_logreg(k, n, model, X.astype(np.float64), guide, params)
    elif form == "strided_view":
        wide = torch.zeros((rows, 2 * d), device="cuda")
        wide[:, 1::2] = Xt
        view = wide[:, 1::2]
        assert not view.is_contiguous()
        got = _run_logreg(k, n, model, view, guide, params)
    elif form == "int32_key":
        k32 = k.view(torch.int32)
        assert k32.dtype == torch.int32
        got = _run_logreg(k32, n, model, Xt, guide, params)
    else:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = _run_logreg(k, n, model, Xt, guide, params)
            got = {s: v.clone() for s, v in got.items()}
        torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert set(got) == set(base)
    for s in base:
        assert got[s].dtype == base[s].dtype and torch.equal(got[s], base[s]), f"{form}: site {s} differs"
