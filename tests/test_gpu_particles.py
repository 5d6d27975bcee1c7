"""Trace_ELBO(num_particles=K) on the device (k_logreg_particles and the particle entry points) against the comparator of
tests/particles_ref.py, which restates the particle key rule on top of the CPU oracle.

Tolerances are those of the single-particle tests: per-example rows PX_RTOL / PX_ATOL of tests/test_gpu_dpsvi.py, trajectories
the production tolerances of tests/test_gpu_production_kernels.py.  On-chip draws equal the stream of d3p_px_eps_sites_particles bit
for bit; that stream agrees with the restated rule to the rtol of d3p_px_eps_sites' own test."""
import numpy as np
import pytest
import torch

from tests import particles_ref as R

pytestmark = pytest.mark.gpu

PX_RTOL, PX_ATOL = 2e-5, 2e-6
LOSS_RTOL, PARAM_RTOL, PARAM_ATOL = 5e-5, 2e-4, 2e-5


def np_(t):
    return t.detach().cpu().numpy()


def _problem(B, d, icpt, gauss, seed, mask_frac=0.75):
    r = np.random.default_rng(seed)
    D = d + int(icpt)
    X = r.normal(size=(B, d)).astype(np.float32)
    if gauss:
        X = (1.0 + 0.5 * X).astype(np.float32)
    y = None if gauss else (r.random(B) < 0.5).astype(np.float32)
    loc = (0.3 * r.normal(size=D)).astype(np.float32)
    unc = (0.5 * r.normal(size=D) - 1.0).astype(np.float32)
    mask = r.random(B) < mask_frac
    mask[0] = True
    if B > 2:
        mask[1] = False
    return X, y, loc, unc, mask


def _svi(d, icpt, gauss, guide, K, N=1000, optim=None, sigma=0.8, lr=1e-2, rng_suite=None):
    import d3p_amd.random as strong
    from d3p_amd.models import (Adam, AutoDiagonalNormal, DiagonalNormalGuide, GaussianMean, LogisticRegression, MeanFieldGuide,
                                Trace_ELBO)
    from d3p_amd.svi import DPSVI
    if gauss:
        model = GaussianMean(d, prior_scale=1.5, obs_scale=0.7)
        g = AutoDiagonalNormal(model) if guide == "auto" else DiagonalNormalGuide(model)
        kw = {"d": d}
    else:
        model = LogisticRegression(d, prior_scale=1.5, intercept=icpt, intercept_prior_scale=3.0)
        g = MeanFieldGuide(model) if guide == "meanfield" else AutoDiagonalNormal(model)
        kw = {}
    loss = Trace_ELBO() if K is None else Trace_ELBO(num_particles=K)
    return DPSVI(model, g, optim or Adam(lr), loss, 1.0, sigma, rng_suite=rng_suite or strong, num_obs_total=N, **kw)


def _spec(O, d, icpt, gauss, guide, N=1000):
    if gauss:
        return O.gauss_mean_spec(d, prior=1.5, lik_sigma=0.7, lik_scale=N, obs_scale=N, guide_exp=guide != "auto")
    return O.logreg_spec(d, icpt, 1.5, 3.0, lik_scale=N, obs_scale=N, guide_exp=guide == "meanfield")


def _state(svi, key, params, N=1000):
    from d3p_amd.svi import DPSVIState
    return DPSVIState(svi.optim.init(torch.tensor(params).cuda()), key, float(N))


def _args(X, y):
    Xt = torch.tensor(X).cuda()
    return (Xt,) if y is None else (Xt, torch.tensor(y).cuda())


def _px_case(O, B, d, icpt, gauss, guide, K, seed, onchip):
    """Per-example rows and losses of the device vs the comparator; returns the device rows."""
    import d3p_amd.random as rng
    X, y, loc, unc, mask = _problem(B, d, icpt, gauss, seed)
    D = d + int(icpt)
    svi = _svi(d, icpt, gauss, guide, K)
    key = rng.PRNGKey(seed)
    st = _state(svi, key, np.concatenate([loc, unc]))
    jk = O.convert_to_jax_rng_key(O.PRNGKey(seed))
    eps = R.px_eps(O, jk, B, D, K) if onchip else np.random.default_rng(seed + 1).normal(size=(B, K, D)).astype(np.float32)
    kw = {} if onchip else {"_eps": torch.tensor(eps).cuda()}
    _, px_loss, px_grads, n, f = svi._compute_per_example_gradients(st, key, *_args(X, y), mask=torch.tensor(mask).cuda(), **kw)
    names = svi.guide.param_names()
    G = np.concatenate([np_(px_grads[names[0]]), np_(px_grads[names[1]])], axis=1)
    eL, eG, en, ef = R.px_grads(O, _spec(O, d, icpt, gauss, guide), loc, unc, X, y, eps, mask.astype(np.float32))
    assert float(n) == en and abs(float(f) - ef) < 1e-6
    np.testing.assert_allclose(G, eG, rtol=PX_RTOL, atol=PX_ATOL * np.abs(eG).max())
    np.testing.assert_allclose(np_(px_loss), eL, rtol=PX_RTOL, atol=PX_ATOL * np.abs(eL).max())
    assert np.all(G[~mask] == 0) and np.all(np_(px_loss)[~mask] == 0)   # masked rows exactly zero
    assert not np.allclose(G[mask], 0)
    return G


# ---------------------------------------------------------------- keys and eps, bit for bit
# (B up to ~300 and K past 8: the key rule at the sizes where the trajectory tests take eps from d3p_px_eps_sites_particles)
@pytest.mark.parametrize("B,K,sizes", [(5, 3, [7, 1]), (4, 2, [513, 1]), (3, 8, [9]), (6, 1, [4, 1]), (300, 9, [37, 1]), (257, 16, [8]),
                                       (64, 33, [13, 1]), (151, 33, [2]), (96, 16, [6, 1]), (299, 9, [4])])
def test_eps_sites_particles_vs_comparator(gpu, O, B, K, sizes):
    import ctypes as C
    import d3p_amd._lib as L
    from d3p_amd._lib import check, ptr, stream_ptr
    jk = O.convert_to_jax_rng_key(O.PRNGKey(B * 10 + K))
    jkd = torch.tensor(np.asarray(jk, np.uint32).view(np.int32)).cuda()
    eps = torch.empty((B, K, sum(sizes)), dtype=torch.float32, device=gpu)
    arr = (C.c_int32 * len(sizes))(*sizes)
    check(L.load().d3p_px_eps_sites_particles(stream_ptr(), ptr(jkd), B, 0, B, K, arr, len(sizes), ptr(eps)))
    # the keys are exact (a wrong key gives unrelated normals); the normals themselves agree with the oracle's stream to the
    # rtol of d3p_px_eps_sites' own test (tests/test_gpu_dpsvi.py: the float32 erf_inv differs from the oracle's in the last ulps)
    np.testing.assert_allclose(np_(eps), R.px_eps_sites(O, jk, B, sizes, K), rtol=2e-6, atol=1e-7)
    if K > 1:   # particle q of example p is a stream of its own
        assert not np.allclose(np_(eps)[:, 0], np_(eps)[:, 1])
    # the rows of a sub-range are those of the whole batch, bit for bit
    part = torch.empty((B - 1, K, sum(sizes)), dtype=torch.float32, device=gpu)
    check(L.load().d3p_px_eps_sites_particles(stream_ptr(), ptr(jkd), B, 1, B - 1, K, arr, len(sizes), ptr(part)))
    assert torch.equal(part, eps[1:])


@pytest.mark.parametrize("gauss,icpt", [(False, True), (False, False), (True, False)])
def test_onchip_particle_eps_equals_restated_eps(gpu, O, gauss, icpt):
    """Single-site guides: gradients with the kernel's own draws equal those with the (B, K, D) eps of d3p_px_eps_sites_particles
    (one site: the same key rule, restated in tests/test_gpu_particles.py::test_eps_sites_particles_vs_comparator), bit for bit."""
    import d3p_amd.random as rng
    B, d, K = 9, 37, 3
    X, y, loc, unc, mask = _problem(B, d, icpt, gauss, 77)
    D = d + int(icpt)
    svi = _svi(d, icpt, gauss, "auto", K)
    key = rng.PRNGKey(77)
    st = _state(svi, key, np.concatenate([loc, unc]))
    eps = _device_eps_fn(K, D)(O.convert_to_jax_rng_key(O.PRNGKey(77)), B)
    mt = torch.tensor(mask).cuda()
    _, l1, g1, _, _ = svi._compute_per_example_gradients(st, key, *_args(X, y), mask=mt)
    _, l2, g2, _, _ = svi._compute_per_example_gradients(st, key, *_args(X, y), mask=mt, _eps=torch.tensor(eps).cuda())
    for k in g1:
        assert torch.equal(g1[k], g2[k])
    assert torch.equal(l1, l2)


# ---------------------------------------------------------------- per-example gradients vs the comparator
@pytest.mark.parametrize("B,d,icpt,gauss,guide,K", [
    (7, 8, False, False, "auto", 2), (13, 5, True, False, "auto", 3), (9, 130, True, False, "auto", 8),
    (33, 520, False, False, "auto", 2), (11, 63, False, True, "auto", 3), (10, 64, False, True, "diag", 2),
    (17, 257, True, False, "auto", 3), (5, 1024, False, False, "auto", 3), (4, 3000, True, False, "auto", 2),
    (3, 1, True, False, "auto", 8)])
@pytest.mark.parametrize("onchip", [False, True])
def test_px_grads_particles_vs_comparator(gpu, O, B, d, icpt, gauss, guide, K, onchip):
    _px_case(O, B, d, icpt, gauss, guide, K, B * 100 + d + K, onchip)


def test_px_grads_particles_at_one_particle_is_the_single_particle_entry(gpu, O):
    """d3p_logreg_px_grads_particles(K = 1) == d3p_logreg_px_grads, bit for bit."""
    import ctypes as C
    import d3p_amd._lib as L
    from d3p_amd._lib import check, ptr, stream_ptr
    B, d = 12, 40
    X, y, loc, unc, mask = _problem(B, d, True, False, 5)
    svi = _svi(d, True, False, "auto", None)
    model = svi._model_struct(d, {}, 1000.0)
    lib = L.load()
    P = 2 * (d + 1)
    Xt, yt = _args(X, y)
    prm = torch.tensor(np.concatenate([loc, unc])).cuda()
    mt = torch.tensor(mask.astype(np.uint8)).cuda()
    jk = torch.tensor(np.asarray(O.convert_to_jax_rng_key(O.PRNGKey(5)), np.uint32).view(np.int32)).cuda()
    outs = []
    for k in (None, 1):
        ws = torch.empty(lib.d3p_logreg_px_grads_workspace(C.byref(model), B), dtype=torch.uint8, device=gpu)
        loss, grads, meta = (torch.empty(B, device=gpu), torch.empty((B, P), device=gpu), torch.empty(2, device=gpu))
        if k is None:
            check(lib.d3p_logreg_px_grads(stream_ptr(), C.byref(model), ptr(prm), ptr(Xt), ptr(yt), ptr(mt), B, None, ptr(jk),
                                          ptr(loss), ptr(grads), ptr(meta), ptr(ws), ws.numel()))
        else:
            check(lib.d3p_logreg_px_grads_particles(stream_ptr(), C.byref(model), ptr(prm), ptr(Xt), ptr(yt), ptr(mt), B, 1, None,
                                                    ptr(jk), ptr(loss), ptr(grads), ptr(meta), ptr(ws), ws.numel()))
        outs.append((loss, grads, meta))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="num_particles"):
        check(lib.d3p_logreg_px_grads_particles(stream_ptr(), C.byref(model), ptr(prm), ptr(Xt), ptr(yt), ptr(mt), B, 0, None,
                                                ptr(jk), ptr(loss), ptr(grads), ptr(meta), ptr(ws), ws.numel()))


# ---------------------------------------------------------------- trajectories
def _compare_traj(new_st, losses, ost, elosses, steps):
    losses = torch.stack([l.reshape(()) for l in losses]) if isinstance(losses, list) else losses
    assert bool(torch.isfinite(losses).all())
    np.testing.assert_allclose(np_(losses), np.asarray(elosses, np.float32), rtol=LOSS_RTOL)
    assert np.array_equal(np_(new_st.rng_key).ravel(), np.asarray(ost.key).ravel())
    assert int(new_st.optim_state[0]) == steps
    np.testing.assert_allclose(np_(new_st.optim_state[1]), ost.params, rtol=PARAM_RTOL, atol=PARAM_ATOL)


@pytest.mark.parametrize("gauss,icpt", [(False, True), (True, False)])
def test_update_trajectory_four_particles(gpu, O, gauss, icpt):
    import d3p_amd.random as rng
    B, d, K, N, steps = 48, 21, 4, 1000, 30
    X, y, loc, unc, mask = _problem(B, d, icpt, gauss, 9)
    D = d + int(icpt)
    svi = _svi(d, icpt, gauss, "auto", K, N)
    loc, unc = np.zeros(D, np.float32), np.full(D, -2.0, np.float32)
    st = _state(svi, rng.PRNGKey(9), np.concatenate([loc, unc]), N)
    spec = _spec(O, d, icpt, gauss, "auto", N)
    hy = O.Hyper(1.0, 0.8, 1e-2, 0.9, 0.999, 1e-8)
    ost = O.LogregState(O.PRNGKey(9), D, loc, unc)
    args = _args(X, y)
    mt = torch.tensor(mask).cuda()
    losses, el = [], []
    for _ in range(steps):
        st, l = svi.update(st, *args, mask=mt)
        losses.append(l)
        el.append(R.update(O, spec, hy, ost, X, y, K, mask.astype(np.float32))[0])
    _compare_traj(st, losses, ost, el, steps)


def test_update_two_call_form_equals_run_form(gpu, O):
    """The two-call form (local sums + finalize, taken when a gradient is requested) and the run form of update agree bit for bit:
    the same kernel, the same workgroup geometry, the same finalize."""
    import d3p_amd.random as rng
    B, d, K = 40, 30, 3
    X, y, loc, unc, mask = _problem(B, d, True, False, 4)
    svi = _svi(d, True, False, "auto", K)
    st = _state(svi, rng.PRNGKey(4), np.concatenate([loc, unc]))
    args = _args(X, y)
    a, la = svi.update(st, *args)
    g = torch.empty(2 * (d + 1), device=gpu)
    b, lb = svi._update_fused(st, *args, _grad_out=g)
    assert torch.equal(la, lb) and torch.equal(a.optim_state[1], b.optim_state[1]) and torch.equal(a.rng_key, b.rng_key)


def _device_eps_fn(K, D):
    """eps of the one-site guides from the device's per-particle draws (the one-site stream is the one-site case of the per-site
    rule; test_eps_sites_particles_vs_comparator shows the kernel equals the restated rule): restating 4096 x K draws per
    step in Python would take minutes for a 140-step run."""
    import ctypes as C
    import d3p_amd._lib as L
    from d3p_amd._lib import check, ptr, stream_ptr

    def fn(jax_key, B):
        jk = torch.tensor(np.asarray(jax_key, np.uint32).view(np.int32)).cuda()
        eps = torch.empty((B, K, D), dtype=torch.float32, device="cuda")
        check(L.load().d3p_px_eps_sites_particles(stream_ptr(), ptr(jk), B, 0, B, K, (C.c_int32 * 1)(D), 1, ptr(eps)))
        return np_(eps)
    return fn


def test_run_steps_feistel_d512_two_particles_across_the_batch_boundary(gpu, O):
    import d3p_amd.random as rng
    from d3p_amd.minibatch import subsample_batchify_data
    N, d, B, K, steps, first = 100_000, 512, 4096, 2, 140, 3
    g = torch.Generator().manual_seed(21)
    X, y = torch.randn(N, d, generator=g), (torch.rand(N, generator=g) < 0.5).float()
    svi = _svi(d, False, False, "auto", K, N, sigma=0.7)
    loc, unc = np.zeros(d, np.float32), np.full(d, -2.0, np.float32)
    st = _state(svi, rng.PRNGKey(3), np.concatenate([loc, unc]), N)
    _, gb = subsample_batchify_data((X.cuda(), y.cuda()), B)
    new_st, losses = svi.run_steps(st, gb, rng.PRNGKey(4), first, steps)
    assert svi.last_run_status() == (False, False)
    spec = O.logreg_spec(d, False, 1.5, 3.0, lik_scale=N, obs_scale=N)
    hy = O.Hyper(1.0, 0.7, 1e-2, 0.9, 0.999, 1e-8)
    ost = O.LogregState(O.PRNGKey(3), d, loc, unc)
    Xn, yn = X.numpy(), y.numpy()
    fn = _device_eps_fn(K, d)
    el = []
    for t in range(steps):
        idx = O.feistel_sample(O.fold_in(O.PRNGKey(4), first + t), N, B)
        el.append(R.update(O, spec, hy, ost, Xn[idx], yn[idx], K, eps_fn=fn)[0])
    _compare_traj(new_st, losses, ost, el, steps)


def test_run_steps_poisson_three_particles(gpu, O):
    import scipy.stats
    import d3p_amd.random as rng
    from d3p_amd.minibatch import poisson_batchify_data
    N, d, K, steps, first = 20_000, 64, 3, 130, 1
    q = 600 / N
    maxB = int(scipy.stats.poisson(N * q).ppf(0.99))
    g = torch.Generator().manual_seed(22)
    X, y = torch.randn(N, d, generator=g), (torch.rand(N, generator=g) < 0.5).float()
    svi = _svi(d, True, False, "auto", K, N, sigma=0.7)
    D = d + 1
    loc, unc = np.zeros(D, np.float32), np.full(D, -2.0, np.float32)
    st = _state(svi, rng.PRNGKey(7), np.concatenate([loc, unc]), N)
    _, gb = poisson_batchify_data((X.cuda(), y.cuda()), q, 0.99)
    new_st, losses = svi.run_steps(st, gb, rng.PRNGKey(8), first, steps)
    assert svi.last_run_status() == (False, False)
    spec = O.logreg_spec(d, True, 1.5, 3.0, lik_scale=N, obs_scale=N)
    hy = O.Hyper(1.0, 0.7, 1e-2, 0.9, 0.999, 1e-8)
    ost = O.LogregState(O.PRNGKey(7), D, loc, unc)
    Xn, yn = X.numpy(), y.numpy()
    fn = _device_eps_fn(K, D)
    el, counts = [], []
    for t in range(steps):
        idx, nsel, nvalid = O.poisson_select(O.fold_in(O.PRNGKey(8), first + t), np.float32(q), N, maxB)
        counts.append(nvalid)
        mask = (np.arange(maxB) < nvalid).astype(np.float32)
        el.append(R.update(O, spec, hy, ost, Xn[idx], yn[idx], K, mask=mask, eps_fn=fn)[0])
    assert min(counts) < maxB
    _compare_traj(new_st, losses, ost, el, steps)


def test_run_steps_equals_get_batch_and_update(gpu, O):
    """The native loop and get_batch + update, 20 Feistel steps at K = 3: bit for bit.  Both run the same two kernels per step with
    the same workgroup count (B examples either way) and batch position p on the same wavefront; only where row p comes from
    differs (a gathered batch vs the table through the Feistel indices), so every partial sum is taken in the same order."""
    import d3p_amd.random as rng
    from d3p_amd.minibatch import subsample_batchify_data
    N, d, B, K, steps = 5000, 24, 256, 3, 20
    g = torch.Generator().manual_seed(23)
    X, y = torch.randn(N, d, generator=g).cuda(), (torch.rand(N, generator=g) < 0.5).float().cuda()
    svi = _svi(d, True, False, "auto", K, N)
    st0 = _state(svi, rng.PRNGKey(1), np.concatenate([np.zeros(d + 1, np.float32), np.full(d + 1, -2.0, np.float32)]), N)
    _, gb = subsample_batchify_data((X, y), B)
    bstate = rng.PRNGKey(2)
    a, la = svi.run_steps(st0, gb, bstate, 0, steps)
    b, lb = st0, []
    for i in range(steps):
        Xb, yb = gb(i, bstate)
        b, l = svi.update(b, Xb, yb)
        lb.append(l.reshape(()))
    assert torch.equal(la, torch.stack(lb))
    assert torch.equal(a.optim_state[1], b.optim_state[1]) and torch.equal(a.rng_key, b.rng_key)


def test_meanfield_update_three_particles(gpu, O):
    import d3p_amd.random as rng
    B, d, K, N, steps = 32, 19, 3, 1000, 8
    X, y, _, _, mask = _problem(B, d, True, False, 31)
    svi = _svi(d, True, False, "meanfield", K, N)
    st = _state(svi, rng.PRNGKey(31), np.zeros(2 * d + 2, np.float32), N)
    spec = _spec(O, d, True, False, "meanfield", N)
    hy = O.Hyper(1.0, 0.8, 1e-2, 0.9, 0.999, 1e-8)
    ost = O.MeanFieldLogregState(O.PRNGKey(31), d)
    args = _args(X, y)
    mt = torch.tensor(mask).cuda()
    losses, el = [], []
    for _ in range(steps):
        st, l = svi.update(st, *args, mask=mt)
        losses.append(l)
        el.append(R.meanfield_update(O, spec, hy, ost, X, y, K, mask.astype(np.float32))[0])
    _compare_traj(st, losses, ost, el, steps)


def test_sgd_through_the_staged_update(gpu, O):
    import d3p_amd.random as rng
    from d3p_amd.models import SGD
    B, d, K, N, steps, lr = 24, 9, 2, 1000, 5, 1e-3
    X, y, loc, unc, mask = _problem(B, d, False, False, 41)
    svi = _svi(d, False, False, "auto", K, N, optim=SGD(lr))
    st = _state(svi, rng.PRNGKey(41), np.concatenate([loc, unc]), N)
    spec = _spec(O, d, False, False, "auto", N)
    key = np.asarray(O.PRNGKey(41), np.uint32).reshape(16)
    params = np.concatenate([loc, unc])
    args = _args(X, y)
    for _ in range(steps):
        st, l = svi.update(st, *args)
        ks = O.split(key, 3)
        jk = O.convert_to_jax_rng_key(ks[1])
        L, G, n, f = R.px_grads(O, spec, params[:d], params[d:], X, y, R.px_eps(O, jk, B, d, K))
        loss, avg = O.combine(O.clip_rows(G, 1.0), L)
        g = O.perturb(ks[2], avg, [d, d], 0.8, 1.0, float(n), 1.0 / spec.inv_obs, f)
        params = (params - np.float32(lr) * g).astype(np.float32)
        key = np.asarray(ks[0], np.uint32).reshape(16)
        np.testing.assert_allclose(float(l), loss, rtol=LOSS_RTOL)
    np.testing.assert_allclose(np_(st.optim_state[1]), params, rtol=PARAM_RTOL, atol=PARAM_ATOL)


# ---------------------------------------------------------------- evaluate
@pytest.mark.parametrize("gauss,guide", [(False, "auto"), (True, "diag"), (False, "meanfield")])
def test_evaluate_four_particles(gpu, O, gauss, guide):
    import d3p_amd.random as rng
    B, d, K = 30, 12, 4
    icpt = guide == "meanfield"
    X, y, loc, unc, _ = _problem(B, d, icpt, gauss, 51)
    svi = _svi(d, icpt, gauss, guide, K)
    spec = _spec(O, d, icpt, gauss, guide)
    D = d + int(icpt)
    params = np.concatenate([loc, unc]) if guide != "meanfield" else (0.2 * np.random.default_rng(5).normal(size=2 * D)).astype(np.float32)
    st = _state(svi, rng.PRNGKey(51), params)
    got = float(svi.evaluate(st, *_args(X, y)))
    jk = O.convert_to_jax_rng_key(O.split(O.PRNGKey(51), 1)[0])
    if guide == "meanfield":
        want = R.meanfield_evaluate(O, spec, params, X, y, jk, K)
    else:
        want = R.evaluate(O, spec, loc, unc, X, y, jk, K)
    np.testing.assert_allclose(got, want, rtol=LOSS_RTOL)
    one = _svi(d, icpt, gauss, guide, 1)
    assert got != float(one.evaluate(_state(one, rng.PRNGKey(51), params), *_args(X, y)))


# ---------------------------------------------------------------- K = 1 unchanged
def test_one_particle_explicit_equals_default(gpu, O):
    import d3p_amd.random as rng
    from d3p_amd.minibatch import subsample_batchify_data
    N, d, B = 3000, 16, 128
    g = torch.Generator().manual_seed(61)
    X, y = torch.randn(N, d, generator=g).cuda(), (torch.rand(N, generator=g) < 0.5).float().cuda()
    res = []
    for K in (None, 1):
        svi = _svi(d, False, False, "auto", K, N)
        st = _state(svi, rng.PRNGKey(6), np.concatenate([np.zeros(d, np.float32), np.full(d, -2.0, np.float32)]), N)
        _, gb = subsample_batchify_data((X, y), B)
        a, la = svi.run_steps(st, gb, rng.PRNGKey(7), 0, 12)
        b, lb = svi.update(a, X[:B], y[:B])
        res.append((la, lb, a.optim_state[1], b.optim_state[1], svi.evaluate(b, X[:B], y[:B])))
    for u, v in zip(*res):
        assert torch.equal(u, v)


# ---------------------------------------------------------------- seeded sweep
def _sweep_cases():
    r = np.random.default_rng(20261015)
    cases = []
    for i in range(40):
        fam = ["logreg", "logreg", "gauss"][i % 3]
        guide = "auto" if fam == "logreg" or i % 2 else "diag"
        d = int(r.choice([1, 3, 16, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 700]))
        cases.append(dict(i=i, gauss=fam == "gauss", guide=guide, icpt=fam == "logreg" and bool(r.random() < 0.5),
                          K=int(r.integers(2, 9)), d=d, B=int(r.integers(1, 40)),
                          source=["explicit", "px"][int(r.integers(0, 2))]))
    return cases


@pytest.mark.parametrize("c", _sweep_cases(), ids=lambda c: f"case{c['i']}")
def test_particles_sweep(gpu, O, c):
    """Per case either the per-example rows (restated eps) or one update through the run form (on-chip eps), vs the comparator."""
    import d3p_amd.random as rng
    seed = 1000 + c["i"]
    if c["source"] == "px":
        _px_case(O, c["B"], c["d"], c["icpt"], c["gauss"], c["guide"], c["K"], seed, onchip=False)
        return
    B, d, K, N = c["B"], c["d"], c["K"], 1000
    X, y, _, _, mask = _problem(B, d, c["icpt"], c["gauss"], seed)
    D = d + int(c["icpt"])
    svi = _svi(d, c["icpt"], c["gauss"], c["guide"], K, N)
    loc, unc = np.zeros(D, np.float32), np.full(D, -2.0, np.float32)
    st = _state(svi, rng.PRNGKey(seed), np.concatenate([loc, unc]), N)
    new_st, l = svi.update(st, *_args(X, y), mask=torch.tensor(mask).cuda())
    ost = O.LogregState(O.PRNGKey(seed), D, loc, unc)
    el = R.update(O, _spec(O, d, c["icpt"], c["gauss"], c["guide"], N), O.Hyper(1.0, 0.8, 1e-2, 0.9, 0.999, 1e-8), ost, X, y, K,
                  mask.astype(np.float32))[0]
    _compare_traj(new_st, [l], ost, [el], 1)
