"""Linear and Poisson regression (D3P_FAMILY_LINREG / D3P_FAMILY_POISSON) on the device against tests/glm_ref.py: the per-example
ELBO of ``torch.distributions`` in float64 with autograd, the oracle's noise streams, and the oracle's own clip / mean / perturbation /
Adam stages.  tests/test_glm_host.py checks that comparator against the oracle's pinned logistic rows on the CPU.

Tolerances are the project's, not the new code's: per-example rows and losses 2e-5 (Poisson gradient rows:
1.4e-4, four times the float32 error of the reference itself on these inputs, tests/glm_ref.py), batch
gradients 1e-4 (+ 1e-6 max), parameters after Adam 1e-5, 20-step trajectories 5e-5 (losses) / 2e-4 (parameters), keys bit-exact.
Inputs: X ~ N(0, 1) / sqrt(d), |loc| = 1.5, so |t| <= 4 (asserted on the float64 side of every per-example comparison)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import glm_ref as R

pytestmark = pytest.mark.gpu

FAMILIES = ("linear", "poisson")
SIGMA = R.SWEEP_SIGMA
WIDTHS = R.SWEEP_WIDTHS


def np_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def rng(gpu):
    import d3p_amd.random as r
    return r


def make_model(family, d, intercept, sigma=None, **kw):
    from d3p_amd.models import LinearRegression, PoissonRegression
    if family == "linear":
        return LinearRegression(d, prior_scale=1.5, intercept=intercept, intercept_prior_scale=2.5,
                                obs_scale=SIGMA["linear"] if sigma is None else sigma)
    return PoissonRegression(d, prior_scale=1.5, intercept=intercept, intercept_prior_scale=2.5, **kw)


def make_svi(family, d, intercept, N, guide="softplus", C_=1.0, dp=1.0, lr=1e-3, K=1, optim=None, sigma=None):
    from d3p_amd.models import Adam, AutoDiagonalNormal, DiagonalNormalGuide, Trace_ELBO
    from d3p_amd.svi import DPSVI
    model = make_model(family, d, intercept, sigma)
    g = AutoDiagonalNormal(model) if guide == "softplus" else DiagonalNormalGuide(model)
    return DPSVI(model, g, optim or Adam(lr), Trace_ELBO(num_particles=K), C_, dp, num_obs_total=N)


def hyper_of(family, d, intercept, N, obs_scale=None, sigma=None):
    return R.hyper(d, intercept, prior_w=1.5, prior_b=2.5, lik_scale=N, obs_scale=N if obs_scale is None else obs_scale,
                   sigma=SIGMA[family] if sigma is None else sigma)


def state_with(svi, key, loc, unc, N):
    from d3p_amd.svi import DPSVIState
    return DPSVIState(svi.optim.init(torch.tensor(np.concatenate([loc, unc]), device="cuda")), key, float(N))


def px_names(guide):
    return ("auto_loc", "auto_scale") if guide == "softplus" else ("w_loc", "w_std_log")


def check_px(got_L, got_G, L, G, family, what):
    """The project's per-example check, as tests/test_gpu_dpsvi.py and tests/test_gpu_gauss.py state it: rtol 2e-5 with an absolute
    floor of 2e-6 of the largest entry.  (A bound relative to each ROW's own scale is not what float32 can give the linear family: a
    row whose residual t - y nearly cancels has a gradient far below its terms, and fl(t - y) carries eps |t| / |t - y|.)  The
    row-scale figures are printed for the record."""
    tol = R.PX_TOL
    gtol = R.POISSON_GRAD_TOL if family == "poisson" else R.PX_TOL      # (calibrated on the CPU: tests/glm_ref.py)
    eg, el = R.row_errors(got_G, G).max(), R.row_errors(got_L, L).max()
    print(f"{what}: worst error relative to the row's scale: gradients {eg:.3e}, losses {el:.3e}")
    np.testing.assert_allclose(got_G, G, rtol=gtol, atol=0.1 * gtol * np.abs(G).max(), err_msg=what)
    np.testing.assert_allclose(got_L, L, rtol=tol, atol=0.1 * tol * np.abs(L).max(), err_msg=what)


# ---------------------------------------------------------------- per-example rows at every kernel form
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_px_grads_at_every_width(rng, O, family, d, intercept):
    """B in {1, 33, 200, 4096 (d <= 512)} with a mask; the guide transform and the noise source (memory / keys) alternate over the
    batch sizes and start from another combination at every (d, intercept), so each width meets all four combinations' kernels."""
    N = R.SWEEP_N
    D = d + int(intercept)
    for B, guide, onchip, seed, X, y, loc, unc, mask, eps in R.sweep_cases(O, family, d, intercept):
        svi = make_svi(family, d, intercept, N, guide)
        key = rng.PRNGKey(seed)
        st = state_with(svi, key, loc, unc, N)
        kw = {} if onchip else {"_eps": torch.tensor(eps).cuda()}
        _, px_loss, px_grads, n, f = svi._compute_per_example_gradients(st, key, torch.tensor(X).cuda(), torch.tensor(y).cuda(),
                                                                        mask=torch.tensor(mask).cuda(), **kw)
        names = px_names(guide)
        assert tuple(sorted(px_grads)) == names
        L, G, en, ef, tmax = R.px_loss_grads(family, R.sweep_hyper(family, d, intercept), loc, unc, X, y, eps, mask, guide, return_t=True)
        assert tmax <= 4.0, tmax
        assert float(n) == en and abs(float(f) - ef) < 1e-6
        got_G = np.concatenate([np_(px_grads[names[0]]), np_(px_grads[names[1]])], axis=1)
        check_px(np_(px_loss), got_G, L, G, family, f"{family} d={d} icpt={intercept} B={B} {guide} {'keys' if onchip else 'memory'}")
        assert np.all(got_G[~mask] == 0) and np.all(np_(px_loss)[~mask] == 0)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("guide", ["softplus", "exp"])
@pytest.mark.parametrize("onchip", [False, True])
@pytest.mark.parametrize("d,intercept", [(4, True), (257, False), (1024, False), (2056, True)])
def test_px_grads_guides_and_noise_sources(rng, O, family, guide, onchip, d, intercept):
    N, B = 5000, 33
    D = d + int(intercept)
    X, y, loc, unc = R.problem(family, B, d, intercept, d + 7, SIGMA[family])
    svi = make_svi(family, d, intercept, N, guide)
    key = rng.PRNGKey(d)
    st = state_with(svi, key, loc, unc, N)
    eps = O.px_eps(O.convert_to_jax_rng_key(O.PRNGKey(d)), B, D) if onchip else np.random.default_rng(3).normal(size=(B, D)).astype(np.float32)
    kw = {} if onchip else {"_eps": torch.tensor(eps).cuda()}
    _, px_loss, px_grads, n, f = svi._compute_per_example_gradients(st, key, torch.tensor(X).cuda(), torch.tensor(y).cuda(), **kw)
    L, G, en, ef, tmax = R.px_loss_grads(family, hyper_of(family, d, intercept, N), loc, unc, X, y, eps, None, guide, return_t=True)
    assert tmax <= 4.0 and float(n) == B and float(f) == 1.0
    names = px_names(guide)
    check_px(np_(px_loss), np.concatenate([np_(px_grads[names[0]]), np_(px_grads[names[1]])], axis=1), L, G, family, f"{family} d={d} {guide}")


@pytest.mark.parametrize("family", FAMILIES)
def test_all_false_mask_is_the_empty_batch(rng, family):
    """n = 0: zero rows from the materialising stage; NaN gradients and the empty_batch_loss rule (0 while the parameters are finite)
    from the fused update."""
    B, d, N = 8, 16, 100
    X, y, loc, unc = R.problem(family, B, d, False, 5, SIGMA[family])
    svi = make_svi(family, d, False, N)
    st = state_with(svi, rng.PRNGKey(1), loc, unc, N)
    none = torch.zeros(B, dtype=torch.bool, device="cuda")
    _, px_loss, px_grads, n, f = svi._compute_per_example_gradients(st, rng.PRNGKey(1), torch.tensor(X).cuda(), torch.tensor(y).cuda(), mask=none)
    assert float(n) == 0 and float(f) == 0 and bool((px_loss == 0).all()) and all(bool((g == 0).all()) for g in px_grads.values())
    gout = torch.empty(2 * d, device="cuda")
    _, loss = svi._update_fused(st, torch.tensor(X).cuda(), torch.tensor(y).cuda(), mask=none, _grad_out=gout)
    assert float(loss) == 0.0 and bool(torch.isnan(gout).all())


# ---------------------------------------------------------------- update
def compare_state(new_st, ref, steps, rtol, atol):
    """Key and step counter bit-exact; parameters at the caller's (the project's) tolerance.  The Adam moments have no figure of their
    own in DESIGN.md section 2: m is linear in the batch gradients, so it takes their bound (1e-4, atol 1e-6 max; trajectories: the
    parameters' 2e-4, atol 2e-5 max), v is quadratic in them, so twice that."""
    assert np.array_equal(np_(new_st.rng_key).ravel(), ref.key)
    assert int(new_st.optim_state[0]) == steps == ref.step
    np.testing.assert_allclose(np_(new_st.optim_state[1]), ref.params, rtol=rtol, atol=atol)
    mr, ma = (1e-4, 1e-6) if steps == 1 else (2e-4, 2e-5)
    np.testing.assert_allclose(np_(new_st.optim_state[2]), ref.m, rtol=mr, atol=ma * np.abs(ref.m).max())
    np.testing.assert_allclose(np_(new_st.optim_state[3]), ref.v, rtol=2 * mr, atol=2 * ma * np.abs(ref.v).max())


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("guide", ["softplus", "exp"])
@pytest.mark.parametrize("B,d,intercept,masked,onchip", [(16, 4, False, False, True), (50, 96, True, True, False), (64, 512, False, False, True),
                                                         (200, 513, True, True, True), (12, 1500, False, True, True), (9, 2600, True, False, False)])
def test_fused_update_vs_reference(rng, O, family, guide, B, d, intercept, masked, onchip):
    """update through the fused kernels (the two-kernel form with _grad_out; the last two shapes: the column-chunked kernel)."""
    N = 5000
    D = d + int(intercept)
    X, y, loc, unc = R.problem(family, B, d, intercept, 7 * B + d, SIGMA[family])
    mask = (np.random.default_rng(6).random(B) < 0.7) if masked else None
    svi = make_svi(family, d, intercept, N, guide, C_=0.7, dp=1.3, lr=1e-2)
    st = state_with(svi, rng.PRNGKey(4242), loc, unc, N)
    eps = None if onchip else np.random.default_rng(2).normal(size=(B, D)).astype(np.float32)
    gout = torch.empty(2 * D, device="cuda")
    new_st, loss = svi._update_fused(st, torch.tensor(X).cuda(), torch.tensor(y).cuda(), mask=torch.tensor(mask).cuda() if masked else True,
                                     _eps=None if onchip else torch.tensor(eps).cuda(), _grad_out=gout)
    ref = R.State(O.PRNGKey(4242), loc, unc)
    hy = O.Hyper(0.7, 1.3, 1e-2, 0.9, 0.999, 1e-8)
    eloss, egrad = R.step(O, family, hyper_of(family, d, intercept, N), hy, ref, X, y, mask, guide, eps=eps)
    np.testing.assert_allclose(np_(gout), egrad, rtol=1e-4, atol=1e-6 * np.abs(egrad).max())
    assert abs(float(loss) - eloss) <= 2e-5 * abs(eloss) + 1e-6
    compare_state(new_st, ref, 1, 1e-5, 1e-6)
    # the one-launch form (update's default route) walks the same step
    st1, loss1 = svi.update(st, torch.tensor(X).cuda(), torch.tensor(y).cuda(), mask=torch.tensor(mask).cuda() if masked else True) \
        if onchip else (None, None)
    if onchip:
        assert abs(float(loss1) - eloss) <= 2e-5 * abs(eloss) + 1e-6
        compare_state(st1, ref, 1, 1e-5, 1e-6)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,d,intercept", [(128, 512, False), (40, 65, True), (10, 2100, False)])
def test_fused_equals_staged(rng, family, B, d, intercept):
    N = 10 ** 5
    X, y, loc, unc = R.problem(family, B, d, intercept, 3, SIGMA[family])
    mask = torch.tensor(np.random.default_rng(4).random(B) < 0.9).cuda()
    svi = make_svi(family, d, intercept, N)
    st = state_with(svi, rng.PRNGKey(77), loc, unc, N)
    Xt, yt = torch.tensor(X).cuda(), torch.tensor(y).cuda()
    s1, l1 = svi.update(st, Xt, yt, mask=mask)
    s2, l2 = svi._update_staged(st, Xt, yt, mask=mask)
    assert torch.equal(s1.rng_key, s2.rng_key)
    assert abs(float(l1) - float(l2)) <= 2e-5 * abs(float(l2))
    np.testing.assert_allclose(np_(s1.optim_state[1]), np_(s2.optim_state[1]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(np_(s1.optim_state[2]), np_(s2.optim_state[2]), rtol=1e-4, atol=1e-6 * float(s2.optim_state[2].abs().max()))
    np.testing.assert_allclose(np_(s1.optim_state[3]), np_(s2.optim_state[3]), rtol=2e-4, atol=2e-6 * float(s2.optim_state[3].abs().max()))
    assert int(s1.optim_state[0]) == int(s2.optim_state[0]) == 1


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("optim", ["sgd", "adadp"])
def test_staged_optimisers_vs_reference(rng, O, family, optim):
    """SGD and ADADP go through d3p_logreg_px_grads and the five stages: two steps (ADADP: one even, one odd) against the comparator's
    rows and the oracle's clip / mean / perturbation / optimiser, as tests/test_gpu_adadp.py::test_dpsvi_with_adadp does for logistic."""
    from d3p_amd.models import SGD
    from d3p_amd.optimizers import ADADP
    from d3p_amd.svi import DPSVIState
    B, d, N, D = 24, 16, 500, 17
    X, y, loc, unc = R.problem(family, B, d, True, 9, SIGMA[family])
    svi = make_svi(family, d, True, N, dp=0.5, optim=SGD(1e-2) if optim == "sgd" else ADADP(1e-2, tol=1.0))
    p0 = np.concatenate([loc, unc]).astype(np.float32)
    st = DPSVIState(svi.optim.init(torch.tensor(p0).cuda()), rng.PRNGKey(1), float(N))
    h = hyper_of(family, d, True, N)
    key = O.PRNGKey(1)
    ox, olr, oxs, oxp = p0.copy(), 1e-2, np.zeros(2 * D, np.float32), p0.copy()
    for i in range(2):
        st, loss = svi.update(st, torch.tensor(X).cuda(), torch.tensor(y).cuda())
        ks = O.split(key, 3)
        key = ks[0]
        eps = O.px_eps(O.convert_to_jax_rng_key(ks[1]), B, D)
        L, G, n, f = R.px_loss_grads(family, h, ox[:D], ox[D:], X, y, eps)
        eloss, avg = O.combine(O.clip_rows(G.astype(np.float32), 1.0), L.astype(np.float32))
        g = O.perturb(ks[2], avg, [D, D], 0.5, 1.0, float(n), float(N), f)
        if optim == "sgd":
            ox = (ox - np.float32(1e-2) * g).astype(np.float32)
        else:
            ox, olr, oxs, oxp = O.adadp(ox, olr, oxs, oxp, g, i, tol=1.0)
        assert abs(float(loss) - eloss) <= 2e-5 * abs(eloss)
        np.testing.assert_allclose(np_(svi.get_params(st)["auto_loc"]), ox[:D], rtol=1e-4, atol=1e-5)
    assert np.array_equal(np_(st.rng_key).ravel(), np.asarray(key).ravel())


# ---------------------------------------------------------------- run_steps
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("sampler", ["feistel", "poisson"])
@pytest.mark.parametrize("d,intercept,B", [(4, False, 200), (512, True, 4096), (2056, False, 64)])
def test_run_steps_vs_reference(rng, O, family, sampler, d, intercept, B):
    from d3p_amd.minibatch import poisson_batchify_data, subsample_batchify_data
    import d3p_amd._lib as L
    steps, N = 20, max(3 * B, 1000)
    X, y, loc, unc = R.problem(family, N, d, intercept, 31 + d, SIGMA[family])
    loc, unc = (0.2 * loc).astype(np.float32), np.full_like(unc, -2.0)
    Xt, yt = torch.tensor(X).cuda(), torch.tensor(y).cuda()
    svi = make_svi(family, d, intercept, N, C_=1.0, dp=0.5, lr=1e-2)
    st = state_with(svi, rng.PRNGKey(100), loc, unc, N)
    q = B / N
    if sampler == "feistel":
        init, get_batch = subsample_batchify_data((Xt, yt), B)
        maxB = B
    else:
        maxB = int(B * 1.2)
        init, get_batch = poisson_batchify_data((Xt, yt), q, maxB)
    _, bstate = init(rng.PRNGKey(200))
    first = 2
    new_st, losses = svi.run_steps(st, get_batch, bstate, first, steps)

    ref = R.State(O.PRNGKey(100), loc, unc)
    hy = O.Hyper(1.0, 0.5, 1e-2, 0.9, 0.999, 1e-8)
    h = hyper_of(family, d, intercept, N)
    elosses = []
    for t in range(steps):
        bk = O.fold_in(O.PRNGKey(200), first + t)
        if sampler == "feistel":
            idx, mask = O.feistel_sample(bk, N, B), None
        else:
            idx, nsel, nvalid = O.poisson_select(bk, np.float32(q), N, maxB)
            mask = (np.arange(maxB) < nvalid).astype(np.float32)
        elosses.append(R.step(O, family, h, hy, ref, X[idx], y[idx], mask)[0])
    np.testing.assert_allclose(np_(losses), elosses, rtol=5e-5)
    compare_state(new_st, ref, steps, 2e-4, 2e-5)
    # one launch per step: the fixed-point sums make it the chained form's result bit for bit
    lib = L.load()
    L.check(lib.d3p_dpvi_logreg_set_run_form(1))
    try:
        st1, losses1 = svi.run_steps(st, get_batch, bstate, first, steps)
    finally:
        L.check(lib.d3p_dpvi_logreg_set_run_form(0))
    assert torch.equal(losses1, losses) and torch.equal(st1.rng_key, new_st.rng_key)
    for a, b in zip(st1.optim_state, new_st.optim_state):
        assert torch.equal(a, b)


# ---------------------------------------------------------------- evaluate
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("guide", ["softplus", "exp"])
@pytest.mark.parametrize("d,intercept", [(33, False), (700, True)])
def test_evaluate_vs_reference(rng, O, family, guide, d, intercept):
    N, B = 10 ** 4, 60
    X, y, loc, unc = R.problem(family, B, d, intercept, 77, SIGMA[family])
    svi = make_svi(family, d, intercept, N, guide)
    st = state_with(svi, rng.PRNGKey(99), loc, unc, N)
    got = float(svi.evaluate(st, torch.tensor(X).cuda(), torch.tensor(y).cuda()))
    jax_key = O.convert_to_jax_rng_key(O.split(O.PRNGKey(99), 1)[0])
    exp = R.evaluate(O, family, hyper_of(family, d, intercept, N, obs_scale=1.0), loc, unc, X, y, jax_key, guide)
    print(f"evaluate {family} d={d}: {got} vs {exp}")
    assert abs(got - exp) <= 2e-5 * abs(exp)


# ---------------------------------------------------------------- particles
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("d", [8, 513])
def test_particles_mean_gradient_rule(rng, O, family, K, d):
    N, B, intercept = 2000, 21, d == 8
    D = d + int(intercept)
    X, y, loc, unc = R.problem(family, B, d, intercept, 5 * d + K, SIGMA[family])
    mask = np.random.default_rng(8).random(B) < 0.8
    svi = make_svi(family, d, intercept, N, K=K, C_=0.9, dp=0.7, lr=1e-2)
    key = rng.PRNGKey(d + K)
    st = state_with(svi, key, loc, unc, N)
    Xt, yt, mt = torch.tensor(X).cuda(), torch.tensor(y).cuda(), torch.tensor(mask).cuda()
    _, px_loss, px_grads, n, f = svi._compute_per_example_gradients(st, key, Xt, yt, mask=mt)
    h = hyper_of(family, d, intercept, N)
    eps = R.px_eps(O, O.convert_to_jax_rng_key(O.PRNGKey(d + K)), B, D, K)
    L, G, en, ef, tmax = R.px_loss_grads(family, h, loc, unc, X, y, eps, mask, return_t=True)
    assert tmax <= 4.0 and float(n) == en
    check_px(np_(px_loss), np.concatenate([np_(px_grads["auto_loc"]), np_(px_grads["auto_scale"])], axis=1), L, G, family, f"{family} K={K} d={d}")
    new_st, loss = svi.update(st, Xt, yt, mask=mt)
    ref = R.State(O.PRNGKey(d + K), loc, unc)
    eloss, _ = R.step(O, family, h, O.Hyper(0.9, 0.7, 1e-2, 0.9, 0.999, 1e-8), ref, X, y, mask, K=K)
    assert abs(float(loss) - eloss) <= 2e-5 * abs(eloss) + 1e-6
    compare_state(new_st, ref, 1, 1e-5, 1e-6)
    got = float(svi.evaluate(st, Xt, yt))
    jk = O.convert_to_jax_rng_key(O.split(O.PRNGKey(d + K), 1)[0])
    exp = float(np.mean([R.evaluate(O, family, hyper_of(family, d, intercept, N, obs_scale=1.0), loc, unc, X, y, k) for k in O.tf_split(jk, K)]))
    assert abs(got - exp) <= 2e-5 * abs(exp)


# ---------------------------------------------------------------- Poisson specifics
def test_poisson_zero_counts(rng, O):
    B, d, N = 40, 20, 1000
    X, _, loc, unc = R.problem("poisson", B, d, True, 12)
    y = np.zeros(B, np.float32)
    y[::3] = 2.0
    svi = make_svi("poisson", d, True, N)
    key = rng.PRNGKey(6)
    st = state_with(svi, key, loc, unc, N)
    _, px_loss, px_grads, n, f = svi._compute_per_example_gradients(st, key, torch.tensor(X).cuda(), torch.tensor(y).cuda())
    eps = O.px_eps(O.convert_to_jax_rng_key(O.PRNGKey(6)), B, d + 1)
    L, G, _, _ = R.px_loss_grads("poisson", hyper_of("poisson", d, True, N), loc, unc, X, y, eps)
    check_px(np_(px_loss), np.concatenate([np_(px_grads["auto_loc"]), np_(px_grads["auto_scale"])], axis=1), L, G, "poisson", "y = 0 rows")


def test_poisson_row_that_overflows_float32_drops_out_of_the_clipped_sum(rng, O):
    """A row whose exp(t) makes the float32 squared norm of its gradient overflow (t = 32 exactly: exp(t) = 7.9e13, times the
    likelihood scale 1e6 / 1, squared: > 3.4e38) has clip factor 1 / max(1, inf / C) = 0 and leaves the clipped sum -- in float32 jax
    as on the device, while a float64 comparator keeps it.  The comparator here is the float32 torch
    restatement of the same ELBO; the loss is the mean of the per-example losses, the overflowing row's finite float32 value included."""
    B, d, N, clip = 16, 8, 10 ** 6, 0.5
    X, y, _, _ = R.problem("poisson", B, d, False, 21)
    loc, unc = np.ones(d, np.float32), np.full(d, -1.0, np.float32)
    X[3] = 4.0                                   # t = 8 * 4 * 1 = 32 exactly (eps = 0 below: z = loc)
    y[3] = 1.0
    eps = np.zeros((B, d), np.float32)
    h = hyper_of("poisson", d, False, N, obs_scale=1.0)
    L32, G32, _, _ = R.px_loss_grads("poisson", h, loc, unc, X, y, eps, dtype=torch.float32)
    G32t = torch.tensor(G32, dtype=torch.float32)
    nrm = (G32t * G32t).sum(1).sqrt()
    assert torch.isinf(nrm[3]) and bool(torch.isfinite(G32t).all()) and int(torch.isinf(nrm).sum()) == 1
    scale = 1.0 / torch.maximum(torch.ones(()), nrm / clip)
    assert float(scale[3]) == 0.0
    avg32 = (G32t * scale[:, None]).sum(0).numpy() / B
    svi = make_svi("poisson", d, False, N, C_=clip, dp=0.0)
    from d3p_amd.svi import DPSVIState
    st = DPSVIState(svi.optim.init(torch.tensor(np.concatenate([loc, unc]), device="cuda")), rng.PRNGKey(2), 1.0)
    gout = torch.empty(2 * d, device="cuda")
    new_st, loss = svi._update_fused(st, torch.tensor(X).cuda(), torch.tensor(y).cuda(), _eps=torch.tensor(eps).cuda(), _grad_out=gout)
    got = np_(gout)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, avg32, rtol=1e-4, atol=1e-6 * np.abs(avg32).max())
    # without that row the sum is the same: it dropped out
    keep = np.arange(B) != 3
    avg_wo = (G32t[keep] * scale[keep, None]).sum(0).numpy() / B
    np.testing.assert_allclose(got, avg_wo, rtol=1e-4, atol=1e-6 * np.abs(avg_wo).max())
    eloss = float(np.mean(L32.astype(np.float32)))
    assert np.isfinite(float(loss)) and abs(float(loss) - eloss) <= 2e-5 * abs(eloss)
    assert bool(torch.isfinite(new_st.optim_state[1]).all())


def test_poisson_row_with_infinite_rate_makes_the_step_non_finite(rng):
    """exp(t) = inf itself (t = 96 > 88.8): the row's loss is +inf and its gradient ENTRIES are infinite, and inf * 0 = NaN in
    float32 jax as here.  The row is not dropped and nothing finite comes out: the loss of the step is not
    finite (the two-kernel form reports the mean of the per-example losses, +inf, as float32 jax does), the gradient and the new
    state are not finite, and a run says so through last_run_status()."""
    from d3p_amd.minibatch import subsample_batchify_data
    B, d, N = 16, 8, 16
    X, y, _, _ = R.problem("poisson", B, d, False, 21)
    loc, unc = np.ones(d, np.float32), np.full(d, -1.0, np.float32)
    X[3] = 12.0                                  # t = 8 * 12 * 1 = 96
    svi = make_svi("poisson", d, False, N, C_=0.5, dp=0.0)
    st = state_with(svi, rng.PRNGKey(2), loc, unc, N)
    Xt, yt = torch.tensor(X).cuda(), torch.tensor(y).cuda()
    eps = torch.zeros((B, d), device="cuda")
    gout = torch.empty(2 * d, device="cuda")
    new_st, loss = svi._update_fused(st, Xt, yt, _eps=eps, _grad_out=gout)      # the two-kernel form
    print("two-kernel form: loss", float(loss))
    assert float(loss) == float("inf")
    assert not bool(torch.isfinite(gout).any()) or bool(torch.isnan(gout).any())
    assert not bool(torch.isfinite(new_st.optim_state[1]).all())
    new_st, loss = svi.update(st, Xt, yt)        # the one-launch form
    print("one-launch form: loss", float(loss))
    assert not np.isfinite(float(loss)) and not bool(torch.isfinite(new_st.optim_state[1]).all())
    init, get_batch = subsample_batchify_data((Xt, yt), B)          # every batch is the whole table: the row is in each
    _, bstate = init(rng.PRNGKey(5))
    run_st, losses = svi.run_steps(st, get_batch, bstate, 0, 3)
    aborted, nonfinite = svi.last_run_status()
    print("run: losses", np_(losses), "status", aborted, nonfinite)
    assert not aborted and nonfinite
    assert not bool(torch.isfinite(losses).any()) and not bool(torch.isfinite(run_st.optim_state[1]).all())


def test_poisson_validate_args(rng):
    B, d, N = 6, 3, 100
    X, y, loc, unc = R.problem("poisson", B, d, False, 2)
    from d3p_amd.models import Adam, AutoDiagonalNormal, PoissonRegression, Trace_ELBO
    from d3p_amd.svi import DPSVI
    model = PoissonRegression(d, validate_args=True)
    svi = DPSVI(model, AutoDiagonalNormal(model), Adam(1e-3), Trace_ELBO(), 1.0, 1.0, num_obs_total=N)
    st = state_with(svi, rng.PRNGKey(1), loc, unc, N)
    Xt = torch.tensor(X).cuda()
    svi.update(st, Xt, torch.tensor(y).cuda())
    for bad in (-1.0, 0.5):
        yb = y.copy()
        yb[2] = bad
        with pytest.raises(ValueError):
            svi.update(st, Xt, torch.tensor(yb).cuda())
        with pytest.raises(ValueError):
            svi.evaluate(st, Xt, torch.tensor(yb).cuda())


# ---------------------------------------------------------------- the C-ABI's refusals
def test_family_validation_in_the_library(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    x = torch.zeros(8, device="cuda")
    for model, rc_want, msg in ((L.LogregModel(4, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LINREG, 0, 0.0), -1, b"lik_sigma"),
                                (L.LogregModel(4, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LINREG, 0, -1.0), -1, b"lik_sigma"),
                                (L.LogregModel(4, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LINREG, 0, float("nan")), -1, b"lik_sigma"),
                                (L.LogregModel(4, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LINREG, 0, float("inf")), -1, b"lik_sigma"),
                                (L.LogregModel(4, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_POISSON, 0, 0.0), -1, b"null label pointer"),
                                (L.LogregModel(4, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LINREG, 0, 1.0), -1, b"null label pointer"),
                                (L.LogregModel(4, 0, 1.0, 1.0, 1.0, 1.0, 4, 0, 0.1), -1, b"unknown likelihood family")):
        labels = None if b"label" in msg else L.ptr(x)
        rc = lib.d3p_logreg_evaluate(None, C.byref(model), L.ptr(x), L.ptr(x), labels, 2, L.ptr(x), L.ptr(x), L.ptr(x), 1 << 20)
        assert rc == rc_want and msg in lib.d3p_last_error(), (rc, lib.d3p_last_error())
    # a row range that is not the whole table (a data-parallel shard) and the two-site guide are refused before any launch
    for fam in (L.D3P_FAMILY_LINREG, L.D3P_FAMILY_POISSON):
        model = L.LogregModel(4, 1, 1.0, 1.0, 1.0, 1.0, fam, 0, 1.0)
        hyper = L.DpsviHyper(1.0, 1.0, 1e-3, 0.9, 0.999, 1e-8)
        keybuf, params, step = torch.zeros(32, dtype=torch.uint32, device="cuda"), torch.zeros(10, device="cuda"), torch.zeros((), dtype=torch.int32, device="cuda")
        st = L.DpsviState(keybuf.data_ptr(), 0, params.data_ptr(), params.data_ptr(), params.data_ptr(), step.data_ptr())
        src = L.BatchSource(L.D3P_BATCH_EXPLICIT, 4, 0.0, 0, None, None, None, 8, 0, 4)
        ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
        sums = torch.full((12,), 7.0, device="cuda")
        rc = lib.d3p_dpvi_logreg_local_sums(None, C.byref(model), C.byref(hyper), C.byref(st), C.byref(src), L.ptr(x), L.ptr(x), None,
                                            L.ptr(sums), L.ptr(ws), ws.numel())
        assert rc not in (0, -1) and b"one GPU" in lib.d3p_last_error(), (rc, lib.d3p_last_error())
        torch.cuda.synchronize()
        assert bool((sums == 7.0).all())
        sites = L.LogregModel(4, 1, 1.0, 1.0, 1.0, 1.0, fam, L.D3P_GUIDE_EXP_SITES, 1.0)
        whole = L.BatchSource(L.D3P_BATCH_EXPLICIT, 4, 0.0, 0, None, None, None, 4, 0, 4)
        rc = lib.d3p_dpvi_logreg_local_sums(None, C.byref(sites), C.byref(hyper), C.byref(st), C.byref(whole), L.ptr(x), L.ptr(x), None,
                                            L.ptr(sums), L.ptr(ws), ws.numel())
        assert rc not in (0, -1) and bool((sums == 7.0).all()), (rc, lib.d3p_last_error())


@pytest.mark.parametrize("name", ["linear_regression", "poisson_regression"])
def test_examples_run_and_learn(gpu, name):
    """examples/linear_regression.py and examples/poisson_regression.py: the loss goes down and loc approaches w_true."""
    import argparse
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ex_" + name, os.path.join(root, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = argparse.Namespace(sigma=0.5, clip_threshold=1.0, num_steps=1500, learning_rate=2e-2, batch_size=200, dimensions=4,
                              num_samples=10000, obs_scale=0.5)
    first, last, err0, err = mod.main(args)
    assert last < first and err < err0
