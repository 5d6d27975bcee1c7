"""CPU reference of predictive sampling (d3p_amd.modelling) for the GPU tests and the `predict` family of tests/fuzz_vs_oracle.py.

Expected draws are rebuilt on the CPU from O.tf_split / O.tf_normal / O.tf_uniform following DESIGN.md section 4b:
  keys = split(key, n) (multi form), posterior: model_key, guide_key = split(draw key), the seed handler's
  `chain, site_key = split(chain)` per key-taking sample statement; Normal: loc + normal * scale; Bernoulli: uniform < p.

Tolerances (stated once, never widened after a failure without a written reason):
  * latent sites: the device computes fl(loc + fl(eps * scale)) in float32 -- two roundings of at most 2^-24 relative each.  Its
    eps agrees with the oracle's normal to the repository's normal() tolerance, rtol 2e-6 / atol 2e-7 (tests/test_gpu_rng.py:
    v_log_f32 on the device, glibc's log1pf in the oracle -- NOT bit for bit); against the float64 value:
    |dev - ref| <= 2e-6 |ref| + (2e-6 |eps| + 2e-7) |scale| + 2^-23 (|loc| + |eps scale|) ("rtol 2e-6 plus one multiply-add").
    Scales that are exp(.) of a parameter add expf's own error (<= 2 ulp) to eps scale.  The two-rounding rule itself is checked
    bit for bit apart from this bound (tests/test_gpu_predictive_edges.py): with the device's own eps, read back through a call
    with loc = 0 and scale = 1, the result must be np.float32(loc) + np.float32(eps) * np.float32(scale) exactly.
  * Bernoulli outcomes: the device compares the float32 uniform u (bit-equal to the oracle's) with a float32 p.  The logit
    x . w + b summed in float32 in ANY order is within gamma_K (sum |x_k w_k| + |b|) of the exact value, gamma_K = (K + 1) 2^-24 /
    (1 - (K + 1) 2^-24) (Higham's bound; doubled here for the +b and the product roundings: (K + 2) 2^-23); the sigmoid is
    1/4-Lipschitz and its float32 evaluation (expf, one add, one divide) adds at most 2^-21.  So an outcome may differ from the
    float64 one only where |u - p64| <= band = gamma (sum |x w| + |b|) / 4 + 2^-21, and must be equal everywhere else.  The
    edge tests and the sweep use the sharp form of the same bound: with E = gamma (sum |x w| + |b|), p32 lies in
    [sigmoid(l - E), sigmoid(l + E)] (the sigmoid is monotone), so band = max(sigmoid(l + E) - p64, p64 - sigmoid(l - E)) + 2^-21
    <= E / 4 + 2^-21; it stays narrow where the logits saturate (|l| > 90), where E / 4 does not.
  * Vacuity guard of that check: `assert_bernoulli` returns the share of outcomes whose |u - p64| falls inside the band (those
    are not checked at all).  A check is only evidence while that share is small: callers assert (assert_not_vacuous) that at most
    VACUITY_MAX = 0.05 of the outcomes, plus two, fall inside.  Calibrated on the CPU with the oracle's latents (the device's draws
    replaced by the oracle's, the outcomes by the float64 ones) over the 2272 logistic cases among seeds 0..2999 of the `predict`
    sweep: the largest share among cases with 200 outcomes or more is 0.0154 (X scaled by 30, d = 1025, logits in the thousands),
    0.0105 with unscaled X; the band's linear form E / 4 would be 1.0 in the first case (140 of the 1818 cases above 0.05).  0.05
    leaves a margin of 3x.
  * VAE: the dense products run on the bf16x3 / fp32 MFMA kernels; per product the error is bounded by the fp32 sum bound with
    a 4x margin for the three-way bf16 split (the dropped lo x lo terms are below 2^-24 relative each): gamma_K = K 2^-22.  The
    bound is propagated layer by layer in float64 (softplus and sigmoid are 1- and 1/4-Lipschitz; softplus' float32 evaluation
    adds 2^-22 (|h| + 1)); z is checked with the propagated encoder bound, the outcomes with the decoder bound evaluated on the
    DEVICE's z.
"""
import numpy as np

from d3p_amd import modelling as M
from d3p_amd.models import AutoDiagonalNormal, MeanFieldGuide

VACUITY_MAX = 0.05


def key(seed):
    import d3p_amd.random.debug as jr
    return jr.PRNGKey(seed)


def key_words(seed):
    """The oracle's form of jax.random.PRNGKey(seed)."""
    seed = int(seed)
    return np.array([(seed >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF], np.uint32)


def np_(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------- CPU restatement of section 4b
def draw_keys(O, key, n, multi):
    return O.tf_split(key, n) if multi else np.asarray(key, np.uint32).reshape(1, 2)


def chains(O, dk, posterior):
    if not posterior:
        return dk, None
    kk = O.tf_split(dk, 2)
    return kk[0], kk[1]


def site_key(O, chain, index):
    c = chain
    for _ in range(index + 1):
        kk = O.tf_split(c, 2)
        c, s = kk[0], kk[1]
    return s


def assert_latent(dev, loc, eps, scale, what):
    ref = loc.astype(np.float64) + eps.astype(np.float64) * scale.astype(np.float64)
    tol = (2e-6 * np.abs(ref) + (2e-6 * np.abs(eps) + 2e-7) * np.abs(scale) + 2.0 ** -23 * (np.abs(loc) + np.abs(eps.astype(np.float64) * scale))
           + 1e-30)
    err = np.abs(dev.astype(np.float64) - ref)
    assert np.all(err <= tol), f"{what}: max err {err.max()} (tol at argmax {tol.ravel()[err.argmax()]})"


def assert_bernoulli(obs, u, p64, band, what):
    """Outcomes equal to the float64 ones outside the band; returns the share of outcomes inside it (the vacuity guard)."""
    obs, u, p64, band = (np.asarray(a) for a in (obs, u, p64, band))
    exp = (u < p64).astype(np.int32)
    inside = np.abs(u - p64) <= band
    bad = (obs != exp) & ~inside
    assert not bad.any(), f"{what}: {int(bad.sum())} outcomes differ outside the band (first at {np.argwhere(bad)[0]})"
    assert set(np.unique(obs)) <= {0, 1}
    return float(inside.mean()) if inside.size else 0.0


def logreg_expect(O, key, n, multi, model, guide, params, X, subst=None):
    """(latent dict, obs keys) rebuilt on the CPU."""
    d = X.shape[1]
    subst = subst or {}
    posterior = guide is not None
    plan = M.site_plan(model, guide, set(subst), d=d, rows=X.shape[0])
    out = {k: [] for k in [s.name for s in plan]}
    okeys = []
    for dk in draw_keys(O, key, n, multi):
        mk, gk = chains(O, dk, posterior)
        for st in plan:
            if st.name == "obs":
                okeys.append(site_key(O, mk, st.key_index))
                continue
            if st.chain == "model" and st.substituted:
                if not posterior:
                    out[st.name].append(np.asarray(subst[st.name], np.float32).reshape(-1))
                continue
            chain = gk if st.chain == "guide" else mk
            eps = O.tf_normal(site_key(O, chain, st.key_index), st.size)
            if posterior:
                if isinstance(guide, AutoDiagonalNormal):
                    loc, sc = params["auto_loc"], params["auto_scale"]
                elif isinstance(guide, MeanFieldGuide):
                    loc, sc = np.atleast_1d(params[st.name + "_loc"]), np.exp(np.atleast_1d(params[st.name + "_std_log"]).astype(np.float64))
                else:
                    loc, sc = params[guide.site + "_loc"], np.exp(params[guide.site + "_std_log"].astype(np.float64))
            else:
                prior = model.intercept_prior_scale if st.name == "intercept" else model.prior_scale
                loc, sc = np.zeros(st.size, np.float32), np.full(st.size, prior)
            out[st.name].append((np.asarray(loc, np.float32), eps, np.asarray(sc, np.float64)))
    return out, okeys


def logreg_band(X64, w, b, d, logit=None):
    """The Bernoulli band of one draw's logits (module docstring).  With `logit` (the float64 logits) the sharp form: the sigmoid is
    monotone, so p32 lies in [sigmoid(logit - E), sigmoid(logit + E)] widened by 2^-21 -- never wider than E / 4 + 2^-21, and far
    narrower where the logits saturate."""
    gamma = (d + 2) * 2.0 ** -23
    E = gamma * (np.abs(X64) @ np.abs(w) + abs(b))
    if logit is None:
        return E / 4 + 2.0 ** -21
    p = expit(logit)
    return np.maximum(expit(logit + E) - p, p - expit(logit - E)) + 2.0 ** -21


def expit(x):
    """1 / (1 + exp(-x)) in float64 without overflow warnings."""
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-x))


def check_logreg(O, res, exp, okeys, X, d, intercept, n, what, sharp=False):
    """Every latent draw and every outcome of every draw; returns the in-band share over all outcomes.  sharp: the band of
    logreg_band's sharp form (tests/test_gpu_predictive_edges.py and the sweep)."""
    for name, draws in exp.items():
        if name == "obs" or not draws:
            continue
        dev = np_(res[name]).reshape(n, -1)
        if isinstance(draws[0], tuple) and draws[0][0].size == d + 1 and name == "w":   # one guide site 'w' over [w | intercept]
            dev = np.concatenate([dev, np_(res["intercept"]).reshape(n, 1)], axis=1)
        for i, dr in enumerate(draws):
            if isinstance(dr, tuple):
                loc, eps, sc = dr
                assert_latent(dev[i], loc, eps, sc, f"{what} {name}[{i}]")
            else:
                assert np.array_equal(dev[i], dr), f"{what}: substituted {name}"
    w = np_(res["w"]).reshape(n, d).astype(np.float64)
    b = np_(res["intercept"]).reshape(n).astype(np.float64) if intercept else np.zeros(n)
    X64 = X.astype(np.float64)
    obs = np_(res["obs"]).reshape(n, -1)
    shares = []
    for i in range(n):
        logit = X64 @ w[i] + b[i]
        band = logreg_band(X64, w[i], b[i], d, logit if sharp else None)
        shares.append(assert_bernoulli(obs[i], O.tf_uniform(okeys[i], X.shape[0]), expit(logit), band, f"{what} obs[{i}]"))
    return float(np.mean(shares))


def assert_not_vacuous(share, count, what=""):
    """The vacuity guard (module docstring): at most VACUITY_MAX of `count` outcomes inside the band, plus two (a handful of outcomes
    cannot be judged)."""
    assert share * count <= VACUITY_MAX * count + 2, f"{what}: {share} of {count} outcomes fall inside the band: the check is vacuous"


def logreg_params(guide, d, intercept, rng):
    D = d + (1 if intercept else 0)
    if isinstance(guide, AutoDiagonalNormal):
        return {"auto_loc": rng.normal(size=D).astype(np.float32), "auto_scale": rng.uniform(0.05, 0.5, D).astype(np.float32)}
    if isinstance(guide, MeanFieldGuide):
        return {"w_loc": rng.normal(size=d).astype(np.float32), "w_std_log": rng.uniform(-3, -0.5, d).astype(np.float32),
                "intercept_loc": np.float32(rng.normal()), "intercept_std_log": np.float32(-1.0)}
    return {guide.site + "_loc": rng.normal(size=D).astype(np.float32), guide.site + "_std_log": rng.uniform(-3, -0.5, D).astype(np.float32)}


# ------------------------------------------------------------------------------- VAE
def vae_net(D, H, Z, H2, rng, scale=0.05):
    from d3p_amd._lib import VaeModel
    shapes, n_dec = M._vae_leaf_shapes(VaeModel(D, H, Z, 1.0, 1.0, H2))
    leaves = [(scale * rng.normal(size=s)).astype(np.float32) for s in shapes]
    nd = n_dec // 2
    dec = []
    for k in range(nd):
        dec += [(leaves[2 * k], leaves[2 * k + 1]), ()]
    enc = []
    ne = (len(shapes) - n_dec - 4) // 2
    for k in range(ne):
        enc += [(leaves[n_dec + 2 * k], leaves[n_dec + 2 * k + 1]), ()]
    Wl, bl, Ws, bs = leaves[-4:]
    enc += [(), ((Wl, bl), ((Ws, bs), ()))]
    layers_dec = [(leaves[2 * k], leaves[2 * k + 1]) for k in range(nd)]
    layers_enc = [(leaves[n_dec + 2 * k], leaves[n_dec + 2 * k + 1]) for k in range(ne)]
    return {"decoder$params": dec, "encoder$params": enc}, layers_dec, layers_enc, (Wl, bl, Ws, bs)


def softplus(x):
    return np.logaddexp(0.0, x)


def dense_bound(h, E, W, b, act):
    """float64 forward of one layer and the propagated bound of its float32 evaluation (module docstring)."""
    W64, b64 = W.astype(np.float64), b.astype(np.float64)
    o = h @ W64 + b64
    K = W.shape[0]
    Eo = E @ np.abs(W64) + K * 2.0 ** -22 * (np.abs(h) @ np.abs(W64) + np.abs(b64))
    if act:
        y = softplus(o)
        return y, Eo + 2.0 ** -22 * (np.abs(y) + 1)
    return o, Eo


def vae_decode_bound(z, layers_dec):
    h, E = z.astype(np.float64), np.zeros(z.shape)
    for k, (W, b) in enumerate(layers_dec):
        h, E = dense_bound(h, E, W, b, k < len(layers_dec) - 1)
    return h, E


def vae_encode_bound(X, layers_enc, heads):
    """(z_loc, its bound, the log of z's scale, its bound) of the encoder in float64."""
    Wl, bl, Ws, bs = heads
    h, E = X.astype(np.float64), np.zeros(X.shape)
    for W, b in layers_enc:
        h, E = dense_bound(h, E, W, b, True)
    zl, El = dense_bound(h, E, Wl, bl, False)
    zs, Es = dense_bound(h, E, Ws, bs, False)
    return zl, El, zs, Es


def vae_posterior_z_ref(zl, El, zs, Es, eps):
    """float64 z = z_loc + eps exp(z_log_scale) and its bound (the encoder's, expf's and the multiply-add's)."""
    ref = zl + eps * np.exp(zs)
    tol = (El + np.abs(eps) * np.exp(zs) * (np.expm1(Es) + 2.0 ** -22) + 2.0 ** -22 * (np.abs(zl) + np.abs(eps) * np.exp(zs))
           + (2e-6 * np.abs(eps) + 2e-7) * np.exp(zs) + 1e-30)
    return ref, tol


def check_vae_obs(O, obs, z_dev, layers_dec, okey, what):
    """One draw's outcomes against the decoder bound evaluated on the device's z; returns the in-band share."""
    logits, Eo = vae_decode_bound(z_dev, layers_dec)
    return assert_bernoulli(obs.ravel(), O.tf_uniform(okey, obs.size), (1 / (1 + np.exp(-logits))).ravel(), (Eo / 4 + 2.0 ** -21).ravel(),
                            what)
