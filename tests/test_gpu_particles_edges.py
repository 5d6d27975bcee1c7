"""k_logreg_particles at the edges of its geometry, against the comparator of tests/particles_ref.py (the float64 CPU oracle).

The kernel sizes its workgroups from LDS (particles_waves): 4 wavefronts while four rows fit, then 2, then 1, and the dynamic-LDS
attribute above 64 KB.  With D = d + intercept:

    stage                                    W = 4      LDS > 64 KB   W = 2        W = 1          refused
    clip-and-accumulate (update, run_steps)  D <= 2044  D >= 819      2045-4088    4089-8178      D >= 8179
    materialising (per-example rows)         D <= 3406  D >= 1365     3407-6814    6815-13630     D >= 13631

Past 1024 * W examples every wavefront loops over several (grid stride).  Tolerances are those of tests/test_gpu_particles.py."""
import numpy as np
import pytest
import torch

from tests import particles_ref as R
from tests.test_gpu_particles import (PX_RTOL, PX_ATOL, _args, _compare_traj, _device_eps_fn, _problem, _spec, _state, _svi,
                                      np_)

pytestmark = pytest.mark.gpu

CLIP_MAX_D, PX_MAX_D = 8178, 13630
HYPER = (1.0, 0.8, 1e-2, 0.9, 0.999, 1e-8)


def _px_rows(O, B, d, icpt, gauss, K, seed, eps_src, guide="auto", params=None, mask=None):
    """Per-example rows and losses (materialising stage) vs the comparator; eps_src: 'onchip' (the kernel's draws; comparator eps
    restated in Python), 'device' (the kernel's draws; comparator eps from d3p_px_eps_sites_particles) or 'random' (explicit eps)."""
    import d3p_amd.random as rng
    X, y, loc, unc, m = _problem(B, d, icpt, gauss, seed)
    mask = m if mask is None else mask
    if params is not None:
        loc, unc = params
    D = d + int(icpt)
    svi = _svi(d, icpt, gauss, guide, K)
    key = rng.PRNGKey(seed)
    st = _state(svi, key, np.concatenate([loc, unc]))
    jk = O.convert_to_jax_rng_key(O.PRNGKey(seed))
    if eps_src == "onchip":
        eps = R.px_eps(O, jk, B, D, K)
    elif eps_src == "device":
        eps = _device_eps_fn(K, D)(jk, B)
    else:
        eps = np.random.default_rng(seed + 1).normal(size=(B, K, D)).astype(np.float32)
    kw = {"_eps": torch.tensor(eps).cuda()} if eps_src == "random" else {}
    _, px_loss, px_grads, n, f = svi._compute_per_example_gradients(st, key, *_args(X, y), mask=torch.tensor(mask).cuda(), **kw)
    names = svi.guide.param_names()
    G = np.concatenate([np_(px_grads[names[0]]), np_(px_grads[names[1]])], axis=1)
    L = np_(px_loss)
    eL, eG, en, ef = R.px_grads(O, _spec(O, d, icpt, gauss, guide), loc, unc, X, y, eps, mask.astype(np.float32))
    assert float(n) == en and abs(float(f) - ef) < 1e-6
    return G, L, eG, eL, mask


def _check_rows(G, L, eG, eL, mask):
    np.testing.assert_allclose(G, eG, rtol=PX_RTOL, atol=PX_ATOL * np.abs(eG).max())
    np.testing.assert_allclose(L, eL, rtol=PX_RTOL, atol=PX_ATOL * np.abs(eL).max())
    assert np.all(G[~mask] == 0) and np.all(L[~mask] == 0)
    assert np.all(np.abs(G[mask]).max(axis=1) > 0)          # every valid row written, none left at zero


def _one_update(O, B, d, icpt, gauss, K, seed, guide="auto", eps_fn=None, unc_center=-2.0, mask=None, loc_unc=None):
    """One update through the run form vs R.update (R.meanfield_update for MeanFieldGuide)."""
    import d3p_amd.random as rng
    X, y, _, _, m = _problem(B, d, icpt, gauss, seed)
    mask = m if mask is None else mask
    D = d + int(icpt)
    svi = _svi(d, icpt, gauss, guide, K)
    hy = O.Hyper(*HYPER)
    spec = _spec(O, d, icpt, gauss, guide)
    if guide == "meanfield":
        st = _state(svi, rng.PRNGKey(seed), np.zeros(2 * D, np.float32))
        ost = O.MeanFieldLogregState(O.PRNGKey(seed), d)
        new_st, l = svi.update(st, *_args(X, y), mask=torch.tensor(mask).cuda())
        el = R.meanfield_update(O, spec, hy, ost, X, y, K, mask.astype(np.float32))[0]
    else:
        if loc_unc is None:
            loc, unc = np.zeros(D, np.float32), np.full(D, unc_center, np.float32)
        else:
            loc, unc = loc_unc
        st = _state(svi, rng.PRNGKey(seed), np.concatenate([loc, unc]))
        ost = O.LogregState(O.PRNGKey(seed), D, loc, unc)
        new_st, l = svi.update(st, *_args(X, y), mask=torch.tensor(mask).cuda())
        el = R.update(O, spec, hy, ost, X, y, K, mask.astype(np.float32), eps_fn=eps_fn)[0]
    return new_st, l, ost, el


# ---------------------------------------------------------------- every workgroup form at its boundaries
@pytest.mark.parametrize("D,icpt,gauss,K,B,eps_src", [
    (1364, False, False, 2, 5, "onchip"), (1365, True, False, 3, 4, "random"), (3406, True, False, 5, 3, "onchip"),
    (3407, False, False, 2, 6, "random"), (6814, False, True, 3, 3, "random"), (6815, True, False, 2, 4, "onchip"),
    (PX_MAX_D, False, False, 3, 3, "random")])
def test_materialising_stage_at_its_form_boundaries(gpu, O, D, icpt, gauss, K, B, eps_src):
    _check_rows(*_px_rows(O, B, D - int(icpt), icpt, gauss, K, 3 * D + K, eps_src))


@pytest.mark.parametrize("D,icpt,gauss,K,B", [
    (818, False, False, 2, 7), (819, True, False, 3, 5), (2044, False, True, 5, 3), (2045, True, False, 2, 6),
    (4088, False, False, 3, 4), (4089, True, False, 2, 5), (CLIP_MAX_D, False, False, 3, 3), (CLIP_MAX_D, True, False, 2, 3)])
def test_clip_stage_at_its_form_boundaries(gpu, O, D, icpt, gauss, K, B):
    new_st, l, ost, el = _one_update(O, B, D - int(icpt), icpt, gauss, K, 5 * D + K)
    _compare_traj(new_st, [l], ost, [el], 1)


def test_meanfield_update_at_the_last_supported_size(gpu, O):
    """MeanFieldGuide's route (_update_leaves: the sites' eps, then the clipped sums) at D = 8178, W = 1."""
    new_st, l, ost, el = _one_update(O, 3, CLIP_MAX_D - 1, True, False, 2, 71, guide="meanfield")
    _compare_traj(new_st, [l], ost, [el], 1)


# ---------------------------------------------------------------- grid stride: several examples per wavefront
@pytest.mark.parametrize("B,d,icpt,gauss,K", [(4097, 20, True, False, 2), (5000, 9, False, True, 3), (9000, 6, False, False, 2),
                                              (2500, 2100, False, False, 2), (1500, 4100, True, False, 2)])
def test_clip_stage_grid_stride(gpu, O, B, d, icpt, gauss, K):
    """W = 4 past 4096 examples, W = 2 (D = 2100) past 2048, W = 1 (D = 4100/4101) past 1024: a wavefront adds several clipped
    rows into its accumulator and carries its loss and count across them."""
    new_st, l, ost, el = _one_update(O, B, d, icpt, gauss, K, B + d, eps_fn=_device_eps_fn(K, d + int(icpt)))
    _compare_traj(new_st, [l], ost, [el], 1)


@pytest.mark.parametrize("B,d,icpt,gauss,K,eps_src", [(5000, 12, True, False, 3, "random"), (4100, 7, False, True, 2, "device"),
                                                      (2500, 3500, False, False, 2, "random"), (1500, 6900, True, False, 2, "random"),
                                                      (1100, 6815, False, False, 2, "device")])
def test_materialising_stage_grid_stride(gpu, O, B, d, icpt, gauss, K, eps_src):
    _check_rows(*_px_rows(O, B, d, icpt, gauss, K, B + d, eps_src))


@pytest.mark.parametrize("gauss", [False, True])
def test_poisson_run_steps_across_the_grid_stride_boundary(gpu, O, gauss):
    """Poisson batches whose capacity is past 1024 * 4 examples (a grid-stride geometry fixed at the capacity) and whose valid count
    falls below 4096 on some steps: the padding positions are masked on every wavefront of the loop."""
    import scipy.stats
    import d3p_amd.random as rng
    from d3p_amd.minibatch import poisson_batchify_data
    N, d, K, steps, first = 12_000, 10, 2, 6, 2
    q = 4100 / N
    maxB = int(scipy.stats.poisson(N * q).ppf(0.99))
    g = torch.Generator().manual_seed(24)
    X = torch.randn(N, d, generator=g)
    if gauss:
        X = 1.0 + 0.5 * X
    y = None if gauss else (torch.rand(N, generator=g) < 0.5).float()
    svi = _svi(d, not gauss, gauss, "auto", K, N, sigma=0.7)
    D = d + int(not gauss)
    loc, unc = np.zeros(D, np.float32), np.full(D, -2.0, np.float32)
    st = _state(svi, rng.PRNGKey(17), np.concatenate([loc, unc]), N)
    table = (X.cuda(),) if gauss else (X.cuda(), y.cuda())
    _, gb = poisson_batchify_data(table, q, 0.99)
    assert int(gb.source.batch_size) == maxB > 4096
    new_st, losses = svi.run_steps(st, gb, rng.PRNGKey(18), first, steps)
    assert svi.last_run_status() == (False, False)
    spec = _spec(O, d, not gauss, gauss, "auto", N)
    ost = O.LogregState(O.PRNGKey(17), D, loc, unc)
    Xn, yn = X.numpy(), None if gauss else y.numpy()
    fn = _device_eps_fn(K, D)
    el, counts = [], []
    for t in range(steps):
        idx, _, nvalid = O.poisson_select(O.fold_in(O.PRNGKey(18), first + t), np.float32(q), N, maxB)
        counts.append(nvalid)
        mask = (np.arange(maxB) < nvalid).astype(np.float32)
        el.append(R.update(O, spec, O.Hyper(1.0, 0.7, 1e-2, 0.9, 0.999, 1e-8), ost, Xn[idx], None if gauss else yn[idx], K,
                           mask=mask, eps_fn=fn)[0])
    assert min(counts) < 4096 < maxB
    _compare_traj(new_st, losses, ost, el, steps)


# ---------------------------------------------------------------- bit-for-bit identities in the new geometries
@pytest.mark.parametrize("B,d,icpt,K", [(5000, 12, True, 3), (1500, 6900, False, 2)])
def test_onchip_draws_equal_eps_from_memory_grid_stride(gpu, O, B, d, icpt, K):
    """Materialising stage, W = 4 and W = 1 past 1024 * W examples: the kernel's draws equal d3p_px_eps_sites_particles' stream."""
    import d3p_amd.random as rng
    X, y, loc, unc, mask = _problem(B, d, icpt, False, 81)
    D = d + int(icpt)
    svi = _svi(d, icpt, False, "auto", K)
    key = rng.PRNGKey(81)
    st = _state(svi, key, np.concatenate([loc, unc]))
    eps = _device_eps_fn(K, D)(O.convert_to_jax_rng_key(O.PRNGKey(81)), B)
    mt = torch.tensor(mask).cuda()
    _, l1, g1, _, _ = svi._compute_per_example_gradients(st, key, *_args(X, y), mask=mt)
    _, l2, g2, _, _ = svi._compute_per_example_gradients(st, key, *_args(X, y), mask=mt, _eps=torch.tensor(eps).cuda())
    for k in g1:
        assert torch.equal(g1[k], g2[k])
    assert torch.equal(l1, l2)


@pytest.mark.parametrize("B,d,icpt,K", [(5000, 12, True, 3), (1500, 4100, False, 2), (1100, 6000, False, 2), (9, 8177, True, 3)])
def test_clip_stage_forms_agree_grid_stride(gpu, O, B, d, icpt, K):
    """Clip-and-accumulate, W = 4 and W = 1 past 1024 * W examples, and rows wider than any single-particle form (D = 6000, 8178):
    the run form of update, the two-call form with on-chip draws and the two-call form with eps from memory (the draws of the
    step's gradient key) agree bit for bit."""
    import d3p_amd.random as rng
    X, y, loc, unc, mask = _problem(B, d, icpt, False, 82)
    D = d + int(icpt)
    svi = _svi(d, icpt, False, "auto", K)
    st = _state(svi, rng.PRNGKey(82), np.concatenate([loc, unc]))
    args = _args(X, y)
    mt = torch.tensor(mask).cuda()
    a, la = svi.update(st, *args, mask=mt)
    g1, g2 = torch.empty(2 * D, device=gpu), torch.empty(2 * D, device=gpu)
    b, lb = svi._update_fused(st, *args, mask=mt, _grad_out=g1)
    jk = O.convert_to_jax_rng_key(O.split(O.PRNGKey(82), 3)[1])
    eps = torch.tensor(_device_eps_fn(K, D)(jk, B)).cuda()
    c, lc = svi._update_fused(st, *args, mask=mt, _eps=eps, _grad_out=g2)
    assert torch.equal(la, lb) and torch.equal(a.optim_state[1], b.optim_state[1]) and torch.equal(a.rng_key, b.rng_key)
    assert torch.equal(lb, lc) and torch.equal(g1, g2) and torch.equal(b.optim_state[1], c.optim_state[1])


@pytest.mark.parametrize("N,d,B,icpt,K", [(12_000, 10, 5000, True, 2), (3000, 4100, 1500, False, 2)])
def test_run_steps_equals_get_batch_and_update_grid_stride(gpu, O, N, d, B, icpt, K):
    import d3p_amd.random as rng
    from d3p_amd.minibatch import subsample_batchify_data
    steps = 3
    g = torch.Generator().manual_seed(25)
    X, y = torch.randn(N, d, generator=g).cuda(), (torch.rand(N, generator=g) < 0.5).float().cuda()
    D = d + int(icpt)
    svi = _svi(d, icpt, False, "auto", K, N)
    st0 = _state(svi, rng.PRNGKey(1), np.concatenate([np.zeros(D, np.float32), np.full(D, -2.0, np.float32)]), N)
    _, gb = subsample_batchify_data((X, y), B)
    bstate = rng.PRNGKey(2)
    a, la = svi.run_steps(st0, gb, bstate, 5, steps)
    b, lb = st0, []
    for i in range(steps):
        Xb, yb = gb(5 + i, bstate)
        b, l = svi.update(b, Xb, yb)
        lb.append(l.reshape(()))
    assert torch.equal(la, torch.stack(lb))
    assert torch.equal(a.optim_state[1], b.optim_state[1]) and torch.equal(a.rng_key, b.rng_key)


# ---------------------------------------------------------------- edge rules at K > 1
def _nan_traj(new_st, l, ost, el):
    """_compare_traj with NaN patterns: loss and parameters NaN where the comparator's are, equal elsewhere."""
    got_l, want_l = float(l), float(el)
    assert np.isnan(got_l) == np.isnan(want_l), (got_l, want_l)
    if not np.isnan(want_l):
        np.testing.assert_allclose(got_l, want_l, rtol=5e-5)
    got_p = np_(new_st.optim_state[1])
    assert np.array_equal(np.isnan(got_p), np.isnan(ost.params)), (int(np.isnan(got_p).sum()), int(np.isnan(ost.params).sum()))
    fin = ~np.isnan(ost.params)
    np.testing.assert_allclose(got_p[fin], ost.params[fin], rtol=2e-4, atol=2e-5)
    assert np.array_equal(np_(new_st.rng_key).ravel(), np.asarray(ost.key).ravel())


@pytest.mark.parametrize("d,icpt,gauss,K", [(9, True, False, 3), (2100, False, False, 2), (6, False, True, 5)])
def test_all_masked_batch(gpu, O, d, icpt, gauss, K):
    B = 7
    new_st, l, ost, el = _one_update(O, B, d, icpt, gauss, K, 91 + d, mask=np.zeros(B, bool))
    _nan_traj(new_st, l, ost, el)


def test_all_masked_batch_meanfield(gpu, O):
    new_st, l, ost, el = _one_update(O, 5, 11, True, False, 3, 92, guide="meanfield", mask=np.zeros(5, bool))
    _nan_traj(new_st, l, ost, el)


@pytest.mark.parametrize("empty", [True, False])
@pytest.mark.parametrize("d,B", [(13, 6), (4100, 5), (20, 4500)])
def test_non_finite_state(gpu, O, empty, d, B):
    """A NaN location: the loss is NaN even when no example is valid (workgroup 0's vote) and the NaN spreads as in the reference."""
    r = np.random.default_rng(d + B)
    D = d + 1
    loc, unc = (0.1 * r.normal(size=D)).astype(np.float32), np.full(D, -2.0, np.float32)
    loc[D // 2] = np.nan
    mask = np.zeros(B, bool) if empty else np.ones(B, bool)
    new_st, l, ost, el = _one_update(O, B, d, True, False, 2, 93, mask=mask, loc_unc=(loc, unc),
                                     eps_fn=_device_eps_fn(2, D) if B > 100 else None)
    assert np.isnan(float(l))
    _nan_traj(new_st, l, ost, el)


@pytest.mark.parametrize("d,B", [(1500, 6), (2001, 4300)])
def test_non_finite_state_rows_mirror_one_particle(gpu, O, d, B):
    """Materialising stage: with a parameter that is not finite every masked example's row and loss are NaN (loss * mask, svi.py:281),
    the rule of the single-particle column-chunked kernel (k_logreg_wide) at these widths; the NaN pattern is K = 1's."""
    import d3p_amd.random as rng
    X, y, loc, unc, mask = _problem(B, d, False, False, 94)
    unc[d // 3] = np.inf
    out = []
    for K in (1, 3):
        svi = _svi(d, False, False, "auto", K)
        st = _state(svi, rng.PRNGKey(94), np.concatenate([loc, unc]))
        _, L, G, n, _ = svi._compute_per_example_gradients(st, rng.PRNGKey(94), *_args(X, y), mask=torch.tensor(mask).cuda())
        names = svi.guide.param_names()
        out.append((np_(L), np.concatenate([np_(G[names[0]]), np_(G[names[1]])], axis=1), float(n)))
    (L1, G1, n1), (L3, G3, n3) = out
    assert n1 == n3 == mask.sum()
    # (valid rows: the infinite scale's column averages +-inf draws over the particles -- NaN at K = 3 where K = 1 keeps an infinity)
    assert np.array_equal(np.isnan(L1), np.isnan(L3)) and np.array_equal(np.isnan(G1[~mask]), np.isnan(G3[~mask]))
    assert np.isnan(L3[~mask]).all() and np.isnan(G3[~mask]).all()


def test_suppressed_first_poisson_batch(gpu, O):
    """handle_oversized_batch='suppress': the run's first batch is empty, the second is not; the trajectory is the comparator's."""
    import scipy.stats
    import d3p_amd.random as rng
    from d3p_amd.minibatch import poisson_batchify_data
    N, d, K, steps, first = 3000, 8, 3, 4, 0
    q = 200 / N
    maxB = int(scipy.stats.poisson(N * q).ppf(0.5))
    bkey = next(k for k in range(1000)
                if O.poisson_select(O.fold_in(O.PRNGKey(k), first), np.float32(q), N, maxB, True)[2] == 0
                and O.poisson_select(O.fold_in(O.PRNGKey(k), first + 1), np.float32(q), N, maxB, True)[2] > 0)
    g = torch.Generator().manual_seed(26)
    X, y = torch.randn(N, d, generator=g), (torch.rand(N, generator=g) < 0.5).float()
    svi = _svi(d, True, False, "auto", K, N, sigma=0.7)
    D = d + 1
    loc, unc = np.zeros(D, np.float32), np.full(D, -2.0, np.float32)
    st = _state(svi, rng.PRNGKey(27), np.concatenate([loc, unc]), N)
    _, gb = poisson_batchify_data((X.cuda(), y.cuda()), q, maxB, handle_oversized_batch="suppress")
    new_st, losses = svi.run_steps(st, gb, rng.PRNGKey(bkey), first, steps)
    spec = _spec(O, d, True, False, "auto", N)
    ost = O.LogregState(O.PRNGKey(27), D, loc, unc)
    Xn, yn = X.numpy(), y.numpy()
    el = []
    for t in range(steps):
        idx, _, nvalid = O.poisson_select(O.fold_in(O.PRNGKey(bkey), first + t), np.float32(q), N, maxB, True)
        mask = (np.arange(maxB) < nvalid).astype(np.float32)
        el.append(R.update(O, spec, O.Hyper(1.0, 0.7, 1e-2, 0.9, 0.999, 1e-8), ost, Xn[idx], yn[idx], K, mask=mask)[0])
    assert svi.last_run_status()[0] is False
    got, el = np_(losses), np.asarray(el, np.float32)
    # (the empty first step's loss is 0; its gradient C / 0 * 0 is NaN, so the state and later losses are NaN)
    assert got[0] == el[0] == 0.0
    assert np.array_equal(np.isnan(got), np.isnan(el))
    np.testing.assert_allclose(got[~np.isnan(el)], el[~np.isnan(el)], rtol=5e-5)
    got_p = np_(new_st.optim_state[1])
    assert np.array_equal(np.isnan(got_p), np.isnan(ost.params))
    assert np.array_equal(np_(new_st.rng_key).ravel(), np.asarray(ost.key).ravel())


@pytest.mark.parametrize("center", [-6.0, -10.0, -14.0])
def test_small_guide_scales(gpu, O, center):
    """Unconstrained scales down to -14 (posterior standard deviations of 8e-7): both stages."""
    r = np.random.default_rng(int(-center))
    d, B, K = 40, 9, 3
    loc = (0.3 * r.normal(size=d + 1)).astype(np.float32)
    unc = (center + 0.3 * r.normal(size=d + 1)).astype(np.float32)
    new_st, l, ost, el = _one_update(O, B, d, True, False, K, 95, loc_unc=(loc, unc))
    _compare_traj(new_st, [l], ost, [el], 1)
    _check_rows(*_px_rows(O, B, d, True, False, K, 96, "onchip", params=(loc, unc)))


# ---------------------------------------------------------------- the refusal
class _Recorder:
    """Stands in for the loaded library: records every entry point looked up except the host-only limit query."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name not in ("d3p_logreg_particles_max_latent", "d3p_last_error", "d3p_abi_version"):
            self.calls.append(name)
        return getattr(self._lib, name)


def _snapshot(st):
    return [t.clone() for t in (st.rng_key,) + tuple(st.optim_state)]


@pytest.mark.parametrize("route", ["update", "update_staged", "run_steps", "px", "meanfield_update", "meanfield_run_steps"])
def test_refusal_before_any_launch(gpu, O, monkeypatch, route):
    import d3p_amd._lib as L
    import d3p_amd.random as rng
    from d3p_amd.minibatch import subsample_batchify_data
    from d3p_amd.models import SGD
    materialising = route in ("px", "update_staged")
    D = (PX_MAX_D if materialising else CLIP_MAX_D) + 1
    meanfield = route.startswith("meanfield")
    d = D - int(meanfield)
    B, N, K = 3, 6, 2
    g = torch.Generator().manual_seed(28)
    X, y = torch.randn(N, d, generator=g).cuda(), (torch.rand(N, generator=g) < 0.5).float().cuda()
    svi = _svi(d, meanfield, False, "meanfield" if meanfield else "auto", K, N, optim=SGD(1e-3) if route == "update_staged" else None)
    st = _state(svi, rng.PRNGKey(29), np.zeros(2 * D, np.float32), N)
    _, gb = subsample_batchify_data((X, y), B)
    bstate = rng.PRNGKey(30)
    torch.cuda.synchronize()
    before = _snapshot(st)
    rec = _Recorder(L.load())
    monkeypatch.setattr(L, "_lib", rec)
    with pytest.raises(L.D3PError, match=str(D - 1)):
        if route in ("update", "update_staged", "meanfield_update"):
            svi.update(st, X[:B], y[:B])
        elif route == "px":
            svi._compute_per_example_gradients(st, rng.PRNGKey(31), X[:B], y[:B])
        else:
            svi.run_steps(st, gb, bstate, 0, 2)
    assert rec.calls == []
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(st)))


@pytest.mark.parametrize("route", ["run_steps", "px"])
def test_last_supported_size_runs(gpu, O, route):
    """run_steps (Feistel, clip stage at D = 8178) and the per-example rows at D = 13630 against the comparator; the update routes at
    these sizes are in the boundary tests above."""
    import d3p_amd.random as rng
    from d3p_amd.minibatch import subsample_batchify_data
    if route == "px":
        _check_rows(*_px_rows(O, 3, PX_MAX_D - 1, True, False, 2, 32, "onchip"))
        return
    N, d, B, K, steps = 8, CLIP_MAX_D, 3, 2, 2
    g = torch.Generator().manual_seed(33)
    X, y = torch.randn(N, d, generator=g), (torch.rand(N, generator=g) < 0.5).float()
    svi = _svi(d, False, False, "auto", K, N)
    loc, unc = np.zeros(d, np.float32), np.full(d, -2.0, np.float32)
    st = _state(svi, rng.PRNGKey(34), np.concatenate([loc, unc]), N)
    _, gb = subsample_batchify_data((X.cuda(), y.cuda()), B)
    new_st, losses = svi.run_steps(st, gb, rng.PRNGKey(35), 0, steps)
    spec = _spec(O, d, False, False, "auto", N)
    ost = O.LogregState(O.PRNGKey(34), d, loc, unc)
    el = []
    for t in range(steps):
        idx = O.feistel_sample(O.fold_in(O.PRNGKey(35), t), N, B)
        el.append(R.update(O, spec, O.Hyper(*HYPER), ost, X.numpy()[idx], y.numpy()[idx], K)[0])
    _compare_traj(new_st, losses, ost, el, steps)
