"""DPSVI.run_steps with the example's own guide (MeanFieldGuide: two sample sites, four parameter leaves) in the native run loop
(D3P_GUIDE_EXP_SITES): against per-step O.meanfield_logreg_update, against the stepwise route, across the 128-step launch boundary,
in the one-launch-per-step form, and as a function of its input state.

Tolerances are those of tests/test_gpu_production_kernels.py: losses rtol 5e-5, final key bit-exact, parameters and Adam moments
rtol 2e-4 / atol 2e-5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_RTOL, PARAM_RTOL, PARAM_ATOL = 5e-5, 2e-4, 2e-5


def np_(t):
    return t.detach().cpu().numpy()


def _table(N, d, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g) * 0.5
    y = (torch.rand(N, generator=g) < 0.5).float()
    return X.contiguous(), y.contiguous()


def _svi(d, N, lr=1e-2, sigma=0.7, clip=1.0):
    from d3p_amd.models import Adam, LogisticRegression, MeanFieldGuide, Trace_ELBO
    from d3p_amd.svi import DPSVI
    model = LogisticRegression(d, prior_scale=1.0, intercept=True, intercept_prior_scale=2.0)
    return DPSVI(model, MeanFieldGuide(model), Adam(lr), Trace_ELBO(), clip, sigma, num_obs_total=N)


def _params(d, seed):
    """A tree-order state away from zero, so that a permutation error shows: [intercept_loc, intercept_std_log, w_loc, w_std_log]."""
    r = np.random.default_rng(seed)
    return np.concatenate([[0.3], [-1.2], 0.2 * r.normal(size=d), -1.0 + 0.3 * r.normal(size=d)]).astype(np.float32)


def _state(svi, d, N, seed):
    import d3p_amd.random as rng
    from d3p_amd.svi import DPSVIState
    return DPSVIState(svi.optim.init(torch.tensor(_params(d, seed)).cuda()), rng.PRNGKey(seed), float(N))


def _oracle(O, d, N, seed, sigma=0.7, lr=1e-2):
    spec = O.logreg_spec(d, True, 1.0, 2.0, lik_scale=N, obs_scale=N, guide_exp=True)
    hy = O.Hyper(1.0, sigma, lr, 0.9, 0.999, 1e-8)
    ost = O.MeanFieldLogregState(O.PRNGKey(seed), d)
    ost.params[:] = _params(d, seed)
    return spec, hy, ost


def _batchifier(X, y, sampler, B):
    import scipy.stats
    from d3p_amd.minibatch import poisson_batchify_data, subsample_batchify_data
    N = X.shape[0]
    if sampler == "feistel":
        return subsample_batchify_data((X.cuda(), y.cuda()), B)[1], B
    q = B / N
    return poisson_batchify_data((X.cuda(), y.cuda()), q, 0.99)[1], int(scipy.stats.poisson(N * q).ppf(0.99))


def _oracle_run(O, spec, hy, ost, X, y, sampler, B, maxB, bseed, first, steps):
    Xn, yn = X.numpy(), y.numpy()
    N = Xn.shape[0]
    losses, counts = [], []
    for t in range(steps):
        bk = O.fold_in(O.PRNGKey(bseed), first + t)
        if sampler == "feistel":
            idx, mask = O.feistel_sample(bk, N, B), None
        else:
            idx, _, nvalid = O.poisson_select(bk, np.float32(B / N), N, maxB)
            mask = (np.arange(maxB) < nvalid).astype(np.float32)
            counts.append(nvalid)
        losses.append(O.meanfield_logreg_update(spec, hy, ost, Xn[idx], yn[idx], mask)[0])
    return np.array(losses, np.float32), counts


def _compare(new_st, losses, ost, el):
    np.testing.assert_allclose(np_(losses), el, rtol=LOSS_RTOL)
    assert np.array_equal(np_(new_st.rng_key).reshape(16), ost.key.reshape(16))
    step, p, m, v = new_st.optim_state
    assert int(step) == ost.step
    np.testing.assert_allclose(np_(p), ost.params, rtol=PARAM_RTOL, atol=PARAM_ATOL)
    np.testing.assert_allclose(np_(m), ost.m, rtol=PARAM_RTOL, atol=PARAM_ATOL)
    np.testing.assert_allclose(np_(v), ost.v, rtol=PARAM_RTOL, atol=PARAM_ATOL)


def _lean_chain_waves(svi, d, N, sampler, B):
    """Waves per workgroup of the lean chain kernel the run loop takes for this shape (0: the generic template)."""
    import ctypes
    import d3p_amd._lib as L
    model = svi._model_struct(d, {}, float(N), sites=True)
    src = L.BatchSource(L.D3P_BATCH_FEISTEL if sampler == "feistel" else L.D3P_BATCH_POISSON, B, B / N, 0, None, None, None, N, 0, N)
    wg, waves = ctypes.c_uint32(0), ctypes.c_int32(0)
    L.check(L.load().d3p_dpvi_logreg_chain_grid(ctypes.byref(model), ctypes.byref(src), 0, ctypes.byref(wg), ctypes.byref(waves)))
    return waves.value


def _count_stepwise(monkeypatch):
    from d3p_amd.svi import DPSVI
    calls = []
    orig = DPSVI._run_steps_stepwise

    def counted(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(DPSVI, "_run_steps_stepwise", counted)
    return calls


def _native_only(monkeypatch):
    from d3p_amd.svi import DPSVI

    def refuse(*a, **k):
        raise AssertionError("run_steps went stepwise")
    monkeypatch.setattr(DPSVI, "_run_steps_stepwise", refuse)


@pytest.mark.parametrize("sampler", ["feistel", "poisson"])
def test_route_is_native(gpu, monkeypatch, sampler):
    import d3p_amd.random as rng
    d, N, B = 16, 5000, 100
    X, y = _table(N, d, 1)
    svi = _svi(d, N)
    st = _state(svi, d, N, 2)
    gb, _ = _batchifier(X, y, sampler, B)
    _native_only(monkeypatch)
    new_st, losses = svi.run_steps(st, gb, rng.PRNGKey(3), 0, 5)
    assert svi.last_run_status() == (False, False)
    assert losses.shape == (5,) and bool(torch.isfinite(losses).all())
    assert int(new_st.optim_state[0]) == 5


@pytest.mark.parametrize("sampler", ["feistel", "poisson"])
def test_production_shape_across_the_launch_boundary_vs_oracle(gpu, O, monkeypatch, sampler):
    """d = 512 + intercept, B = 4096, 140 steps (two prepared batches of the run loop)."""
    import d3p_amd.random as rng
    d, N, B, steps, first = 512, 100_000, 4096, 140, 5
    X, y = _table(N, d, 11)
    svi = _svi(d, N)
    st = _state(svi, d, N, 12)
    gb, maxB = _batchifier(X, y, sampler, B)
    _native_only(monkeypatch)
    assert _lean_chain_waves(svi, d, N, sampler, B) == 16   # the two-site form of the lean chain kernel (k_logreg_chain_sites)
    new_st, losses = svi.run_steps(st, gb, rng.PRNGKey(13), first, steps)
    assert svi.last_run_status() == (False, False)
    spec, hy, ost = _oracle(O, d, N, 12)
    el, counts = _oracle_run(O, spec, hy, ost, X, y, sampler, B, maxB, 13, first, steps)
    if sampler == "poisson":
        assert min(counts) < maxB   # ragged masks
    _compare(new_st, losses, ost, el)


@pytest.mark.parametrize("sampler", ["feistel", "poisson"])
@pytest.mark.parametrize("d,B,steps", [(4, 200, 20), (70, 33, 12), (255, 64, 8), (700, 96, 6), (2048, 64, 6), (2049, 40, 4)])
def test_generic_widths_vs_oracle(gpu, O, monkeypatch, d, B, steps, sampler):
    """Even and odd d (the intercept is the second column of the last w pair, or of a pair of its own), one to eight columns per
    lane; d >= 1024 has rows too wide for the fused step and runs stepwise -- the same result."""
    import d3p_amd.random as rng
    N, first = 4000, 2
    X, y = _table(N, d, 20 + d)
    svi = _svi(d, N)
    st = _state(svi, d, N, 21 + d)
    gb, maxB = _batchifier(X, y, sampler, B)
    stepwise = _count_stepwise(monkeypatch)
    new_st, losses = svi.run_steps(st, gb, rng.PRNGKey(22), first, steps)
    assert bool(stepwise) == (d >= 1024)     # the native loop for every width the fused step serves
    assert svi.last_run_status() == (False, False)
    spec, hy, ost = _oracle(O, d, N, 21 + d)
    el, _ = _oracle_run(O, spec, hy, ost, X, y, sampler, B, maxB, 22, first, steps)
    _compare(new_st, losses, ost, el)


@pytest.mark.parametrize("d,B,sampler", [(512, 4096, "feistel"), (4, 200, "poisson"), (33, 50, "feistel")])
def test_same_trajectory_as_stepwise(gpu, d, B, sampler):
    import d3p_amd.random as rng
    N, steps = 20_000, 9
    X, y = _table(N, d, 30)
    svi = _svi(d, N)
    gb, _ = _batchifier(X, y, sampler, B)
    a, la = svi.run_steps(_state(svi, d, N, 31), gb, rng.PRNGKey(32), 1, steps)
    b, lb = svi._run_steps_stepwise(_state(svi, d, N, 31), gb, rng.PRNGKey(32), 1, steps)
    assert np.array_equal(np_(a.rng_key), np_(b.rng_key))
    np.testing.assert_allclose(np_(la), np_(lb), rtol=1e-4)
    for x, z in zip(a.optim_state[1:], b.optim_state[1:]):
        np.testing.assert_allclose(np_(x), np_(z), rtol=1e-4, atol=1e-5)
    assert int(a.optim_state[0]) == int(b.optim_state[0]) == steps


@pytest.mark.parametrize("d,B", [(512, 4096), (9, 64)])
def test_functional_and_resumable(gpu, d, B):
    import d3p_amd.random as rng
    from d3p_amd.svi import DPSVIState
    N = 20_000
    X, y = _table(N, d, 40)
    svi = _svi(d, N)
    gb, _ = _batchifier(X, y, "feistel", B)
    st = _state(svi, d, N, 41)
    before = [np_(t).copy() for t in st.optim_state[1:]] + [np_(st.rng_key).copy()]
    one, l1 = svi.run_steps(st, gb, rng.PRNGKey(42), 0, 25)
    after = [np_(t) for t in st.optim_state[1:]] + [np_(st.rng_key)]
    assert all(np.array_equal(u, w) for u, w in zip(before, after))            # the input state is untouched
    half, l7 = svi.run_steps(st, gb, rng.PRNGKey(42), 0, 7)
    two, l18 = svi.run_steps(half, gb, rng.PRNGKey(42), 7, 18)                 # continues from the previous run's final key
    # (the split run's step 7 update is applied by k_flush, the whole run's by the next step's prologue: the same expression in two
    #  kernels, which the compiler may round apart by an ulp -- as for every guide; keys and step counts are exact)
    np.testing.assert_allclose(np_(l1), np.concatenate([np_(l7), np_(l18)]), rtol=1e-5)
    for u, w in zip(one.optim_state[1:], two.optim_state[1:]):
        np.testing.assert_allclose(np_(u), np_(w), rtol=1e-5, atol=1e-6)
    assert int(one.optim_state[0]) == int(two.optim_state[0]) == 25
    assert np.array_equal(np_(one.rng_key), np_(two.rng_key))
    # a continuing run equals a run from a freshly built copy of the same state (host-derived first links or not)
    fresh = DPSVIState(tuple(t.clone() for t in half.optim_state), half.rng_key.clone(), half.observation_scale)
    three, l18b = svi.run_steps(fresh, gb, rng.PRNGKey(42), 7, 18)
    assert np.array_equal(np_(l18), np_(l18b))
    for u, w in zip(two.optim_state, three.optim_state):
        assert np.array_equal(np_(u), np_(w))
    assert np.array_equal(np_(two.rng_key), np_(three.rng_key))


@pytest.mark.parametrize("d,B,sampler", [(512, 4096, "feistel"), (70, 33, "poisson")])
def test_one_launch_per_step_form_equals_chained(gpu, d, B, sampler):
    import d3p_amd._lib as L
    import d3p_amd.random as rng
    N, steps = 20_000, 10
    X, y = _table(N, d, 50)
    svi = _svi(d, N)
    gb, _ = _batchifier(X, y, sampler, B)
    a, la = svi.run_steps(_state(svi, d, N, 51), gb, rng.PRNGKey(52), 3, steps)
    lib = L.load()
    L.check(lib.d3p_dpvi_logreg_set_run_form(1))
    try:
        b, lb = svi.run_steps(_state(svi, d, N, 51), gb, rng.PRNGKey(52), 3, steps)
    finally:
        L.check(lib.d3p_dpvi_logreg_set_run_form(0))
    assert svi.last_run_status() == (False, False)
    assert np.array_equal(np_(a.rng_key), np_(b.rng_key))
    np.testing.assert_allclose(np_(la), np_(lb), rtol=1e-5)
    for x, z in zip(a.optim_state[1:], b.optim_state[1:]):
        np.testing.assert_allclose(np_(x), np_(z), rtol=1e-5, atol=1e-6)


def test_get_params_of_a_run(gpu):
    import d3p_amd.random as rng
    d, N, B = 12, 3000, 50
    X, y = _table(N, d, 60)
    svi = _svi(d, N)
    gb, _ = _batchifier(X, y, "feistel", B)
    new_st, _ = svi.run_steps(_state(svi, d, N, 61), gb, rng.PRNGKey(62), 0, 4)
    p = svi.get_params(new_st)
    flat = np_(new_st.optim_state[1])
    assert list(p) == ["intercept_loc", "intercept_std_log", "w_loc", "w_std_log"]
    assert p["intercept_loc"].shape == () and p["intercept_std_log"].shape == ()
    assert p["w_loc"].shape == (d,) and p["w_std_log"].shape == (d,)
    assert float(p["intercept_loc"]) == flat[0] and float(p["intercept_std_log"]) == flat[1]
    assert np.array_equal(np_(p["w_loc"]), flat[2:2 + d]) and np.array_equal(np_(p["w_std_log"]), flat[2 + d:])


def test_empty_batch_turns_the_state_nonfinite(gpu, O, monkeypatch):
    """A Poisson batch with no valid example (factor 0): as in update, the noise scale C / n is infinite and the state turns NaN; the
    next non-empty step's sums are then NaN, which the run reports as non-finite."""
    import d3p_amd.random as rng
    d, N, steps, q = 8, 2000, 12, 5e-4     # one expected example per batch: max batch size 4, about a third of the batches empty
    X, y = _table(N, d, 70)
    svi = _svi(d, N)
    gb, maxB = _batchifier(X, y, "poisson", q * N)
    counts = [O.poisson_select(O.fold_in(O.PRNGKey(72), t), np.float32(q), N, maxB)[2] for t in range(steps)]
    first_empty = counts.index(0)
    assert any(c > 0 for c in counts[first_empty + 1:])   # (the case this test is about)
    _native_only(monkeypatch)
    new_st, losses = svi.run_steps(_state(svi, d, N, 71), gb, rng.PRNGKey(72), 0, steps)
    assert svi.last_run_status() == (False, True)
    assert bool(torch.isfinite(losses[:first_empty]).all())
    assert bool(torch.isnan(new_st.optim_state[1]).all())


@pytest.mark.parametrize("d,B", [(512, 4096), (70, 33)])
def test_non_contiguous_state_runs_in_place_vs_oracle(gpu, O, monkeypatch, d, B):
    """A state whose arrays are views with a stride: run_steps copies it and runs d3p_dpvi_logreg_run in place (the tree-order state
    goes through the workspace's spare rows)."""
    import d3p_amd.random as rng
    from d3p_amd.svi import DPSVIState
    N, steps, first = 20_000, 6, 1
    X, y = _table(N, d, 80)
    svi = _svi(d, N)
    p = torch.tensor(_params(d, 81)).cuda()
    wide = torch.zeros((3, 2 * d + 2, 2), dtype=torch.float32, device="cuda")
    wide[0, :, 0] = p
    st = DPSVIState((svi.optim.init(p)[0], wide[0, :, 0], wide[1, :, 0], wide[2, :, 0]), rng.PRNGKey(81), float(N))
    assert not st.optim_state[1].is_contiguous()
    gb, maxB = _batchifier(X, y, "feistel", B)
    _native_only(monkeypatch)
    new_st, losses = svi.run_steps(st, gb, rng.PRNGKey(82), first, steps)
    assert svi.last_run_status() == (False, False)
    assert np.array_equal(np_(st.optim_state[1]), np_(p))   # the input state is untouched
    spec, hy, ost = _oracle(O, d, N, 81)
    el, _ = _oracle_run(O, spec, hy, ost, X, y, "feistel", B, maxB, 82, first, steps)
    _compare(new_st, losses, ost, el)
