"""The mixture model's production update (k_gmm_px<SUM = true> -> k_gmm_head -> k_gmm_flush, d3p_gmm.hip) where it can be subtly
wrong without the rest of the suite noticing: every other GMM update test starts from `optim.init` (m = v = 0, step 0), where
`b1 m_old`, `b2 v_old` and any read of them are exactly 0.

- The column update (`gmm_apply_column`, `gmm_pending_loss`) bit for bit against a numpy float32 restatement, one rounding per
  operation in the kernel's order, from live Adam moments, through `d3p_dpvi_gmm_apply` with sums chosen by the test.
- The fused update against the float64 oracle chain at every compiled form of the per-example kernel (component pairs per wave,
  64-wide dimension slots, paired or single threefry calls, the full-tile form), at the batch edges of the Dirichlet workgroups
  (256 / K whole examples each) and of the resident grid's stride (4 * 256 * occupancy examples), from a live state.
- The run loop from a live state, across a prepared batch of 64 steps, against stepwise `update()` bit for bit, at forms the
  loop tests of test_gpu_gmm_model.py do not use."""
import numpy as np
import pytest
import torch

from .test_gpu_gmm_model import make_svi, np_, problem

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def rng(gpu):
    import d3p_amd.random as r
    return r


def live_state(key, params, m, v, step, N):
    from d3p_amd.svi import DPSVIState
    cuda = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32)).cuda()   # noqa: E731
    return DPSVIState((torch.tensor(step, dtype=torch.int32).cuda(), cuda(params), cuda(m), cuda(v)), key, float(N))


# ---------------------------------------------------------------------------------------------------------------- A: the column update
def restate_apply(sums, noise, x0, m0, v0, i, B_total, dp_scale, clip, N, lr, b1, b2, eps):
    """gmm_pending_count / gmm_pending_loss / gmm_apply_column of d3p_gmm.hip in numpy float32, one rounding per operation, in the
    kernel's order (numpy's float32 division and square root are correctly rounded, as __fdiv_rn and sqrtf are on the device).  The
    bias terms 1 - b^(i + 1) are exact here: the callers pick b whose powers are exact in float32."""
    P = x0.size
    tot, ls, n = sums[:P], f32(sums[P]), f32(sums[P + 1])
    Bf = f32(B_total)
    obs_scale = f32(1) / f32(1.0 / N)                      # u.obs_scale = 1.0f / model->inv_obs
    b1, b2 = f32(b1), f32(b2)
    bc1 = f32(1) - f32(float(b1) ** (i + 1))
    bc2 = f32(1) - f32(float(b2) ** (i + 1))
    with np.errstate(all="ignore"):
        factor = f32(0) if n == 0 else Bf / n
        noise_scale = f32(dp_scale) * (f32(clip) / n)
        g = (((tot / Bf) + (noise * noise_scale)) * obs_scale) * factor
        m = (f32(1) - b1) * g + b1 * m0
        v = ((f32(1) - b2) * g) * g + b2 * v0
        x = x0 - (f32(lr) * (m / bc1)) / (np.sqrt(v / bc2) + f32(eps))
        loss = ((ls / Bf) * obs_scale) * factor
        # (what a single-rounding fma(noise, noise_scale, tot / B) would give: reported when the kernel differs)
        g_fma = ((((tot / Bf).astype(np.float64) + noise.astype(np.float64) * np.float64(noise_scale)).astype(f32) * obs_scale)
                 * factor)
    return x, m, v, g, f32(loss), g_fma


@pytest.mark.parametrize("count", ["partial", "one", "zero"])
@pytest.mark.parametrize("step", [0, 1, 7, 100_000])
def test_apply_column_bit_for_bit(rng, step, count):
    """d3p_dpvi_gmm_apply (prep -> k_gmm_flush on P + 2 given sums) = the float32 restatement exactly, from live moments.  The noise is
    d3p_amd.random.normal on split(split(state_key, 3)[2], 2) (svi.py:491, :487): sites of K and K d normals."""
    from d3p_amd.dist import GmmHipEngine
    from d3p_amd.models import Adam
    K, d, N, B_total, C, sigma, lr = 16, 64, 10**5, 300, 2.5, 0.7, 1e-2
    # the production b at step 0 (powf(b, 1) = b); later, dyadic b whose powers up to the 8th are exact in float32 (and that
    # underflow to exactly 0 at step 100 000): the test pins the update's roundings, not the device's powf
    b1, b2 = (0.9, 0.999) if step == 0 else (0.5, 0.875)
    n = {"partial": 187, "one": 1, "zero": 0}[count]
    P = K + K * d
    r = np.random.default_rng(1000 + step + {"partial": 0, "one": 1, "zero": 2}[count])
    x0 = (r.normal(size=P) * 2).astype(f32)
    v0 = np.exp(r.uniform(-6, 6, size=P)).astype(f32) * f32(1e6)
    m0 = (r.normal(size=P) * np.sqrt(v0)).astype(f32)
    CB = f32(C) * f32(B_total)
    tot = (r.uniform(-1, 1, size=P) * C * max(n, 1)).astype(f32)
    tot[r.random(P) < 0.1] = 0.0
    tot[:6] = [CB, -CB, np.nextafter(CB, f32(0)), -np.nextafter(CB, f32(0)), 0.0, -0.0]
    sums = np.concatenate([tot, [f32(-123456.789), f32(n)]]).astype(f32)

    svi = make_svi(K, d, N, C=C, sigma=sigma, optim=Adam(lr, b1=b1, b2=b2))
    key = rng.PRNGKey(77 + step)
    st = live_state(key, x0, m0, v0, step, N)
    eng = GmmHipEngine(svi)
    eng.begin(st, torch.zeros((4, d), device="cuda"), B_total, 0)
    gout = torch.full((P,), float("nan"), device="cuda")
    new_st, loss = eng.apply(torch.tensor(sums).cuda(), gout)
    ks = rng.split(key, 3)
    site = rng.split(ks[2], 2)
    noise = np.concatenate([np_(rng.normal(site[0], (K,))), np_(rng.normal(site[1], (K * d,)))]).astype(f32)
    torch.cuda.synchronize()

    x, m, v, g, el, g_fma = restate_apply(sums, noise, x0, m0, v0, step, B_total, sigma, C, N, lr, b1, b2, 1e-8)
    gx, gm, gv, gg = (np_(t).ravel() for t in (new_st.optim_state[1], new_st.optim_state[2], new_st.optim_state[3], gout))
    assert torch.equal(new_st.rng_key.reshape(-1), ks[0].reshape(-1))
    assert int(new_st.optim_state[0]) == step + 1
    if n == 0:   # factor 0 and noise_scale inf (svi.py:305, :365): NaN, as _update_staged gives on an empty batch
        assert np.isnan(g).all() and np.isnan(x).all()
    differ = ~((gg == g) | (np.isnan(gg) & np.isnan(g)))
    fma_like = differ & (gg == g_fma)
    what = (f"step {step}, n {n}: g differs in {int(differ.sum())} of {P} columns ({int((noise[differ] != 0).sum())} with noise != 0); "
            f"{int(fma_like.sum())} of them equal the single-rounding fma(noise, noise_scale, tot / B)")
    for name, got, want in (("g", gg, g), ("x", gx, x), ("m", gm, m), ("v", gv, v)):
        assert np.array_equal(got, want, equal_nan=True), f"{name}: " + what
    assert np.array_equal(np_(loss).reshape(()), el, equal_nan=True), (float(loss), el)


# ------------------------------------------------------------------------------------------------------ C: every form vs float64
def _form(K, d):
    """(KH, DS, PAIRED, FULLT, occupancy) as gmm_launch_px picks them (DS 3 runs the DS = 4 instantiation)."""
    KH = 8 if (K + 1) // 2 <= 8 else 16
    DS = (d + 63) // 64
    DS = 4 if DS == 3 else DS
    DS = 2 if KH == 16 and DS > 1 else DS
    occ = 3 if KH * DS <= 8 else 2 if KH * DS <= 16 else 1
    return KH, DS, K % 2 == 0, K == 2 * KH and d == 64 * DS, occ


# (K, d, B, mask): every (KH, DS, PAIRED, FULLT) form at B = 1 and on the Dirichlet workgroup edges 256 / K, 256 / K + 1; the resident
# grid's first stride (B = 4 * 256 * occ + 1) at one non-full form of each occupancy class; no mask / 70 % / one row kept
FORM_CASES = [
    (1, 1, 1, "none"), (1, 200, 5, "70"), (3, 64, 85, "none"), (3, 64, 86, "one"), (3, 128, 1, "none"), (3, 128, 86, "70"),
    (3, 256, 85, "70"), (3, 256, 86, "none"), (16, 1, 16, "one"), (16, 63, 16, "none"), (16, 63, 17, "70"), (16, 65, 1, "none"),
    (16, 65, 17, "one"), (16, 129, 16, "70"), (16, 200, 17, "none"), (17, 64, 15, "70"), (17, 64, 16, "none"), (17, 128, 1, "none"),
    (17, 128, 16, "one"), (32, 63, 8, "none"), (32, 63, 9, "70"), (32, 65, 9, "none"), (32, 128, 8, "one"),
    # the five full-tile shapes
    (16, 64, 1, "none"), (16, 64, 17, "70"), (16, 128, 16, "none"), (16, 256, 17, "one"), (32, 64, 9, "70"), (32, 128, 8, "none"),
    (32, 128, 9, "70"),
    # three dimension slots run the four-slot form, never its full tile (K = 16, d = 192 once took the d = 256 tile)
    (16, 192, 17, "70"), (16, 192, 1, "none"),
    # the resident grid strides: occupancy 3, 2, 1
    (3, 63, 3073, "70"), (3, 128, 2049, "none"), (3, 200, 1025, "70"),
]


def test_form_cases_cover_every_form():
    forms = {_form(K, d)[:4] for K, d, _, _ in FORM_CASES}
    want = {(KH, DS, pr, False) for KH, DS in ((8, 1), (8, 2), (8, 4), (16, 1), (16, 2)) for pr in (False, True)}
    want |= {(8, 1, True, True), (8, 2, True, True), (8, 4, True, True), (16, 1, True, True), (16, 2, True, True)}
    assert forms == want
    for occ in (1, 2, 3):
        assert any(B == 4 * 256 * occ + 1 and _form(K, d)[4] == occ and not _form(K, d)[3] for K, d, B, _ in FORM_CASES)


@pytest.mark.parametrize("K,d,B,mask_kind", FORM_CASES)
def test_fused_update_vs_oracle_at_every_form(rng, O, K, d, B, mask_kind):
    """_update_gmm_fused from a live state (x, m, v, i) = gmm_px_grads -> clip_rows -> combine -> perturb -> adam(i) of the oracle,
    at the tolerances of test_staged_update_vs_oracle."""
    N, sigma, lr, i = 10**5, 0.5, 1e-2, 3
    P = K + K * d
    X, params = problem(B, K, d, 31 * K + d + B)
    r = np.random.default_rng(7 * K + 3 * d + B)
    mask = {"none": np.ones(B, bool), "70": r.random(B) < 0.7, "one": np.arange(B) == B // 2}[mask_kind]
    mask[B // 2] = True
    seed = 1000 + K * d + B
    spec = O.gmm_spec(K, d, 10.0, lik_scale=N, obs_scale=N)
    ks = O.split(O.PRNGKey(seed), 3)
    L, G, n, f = O.gmm_px_grads(spec, params, X, O.convert_to_jax_rng_key(ks[1]), None if mask_kind == "none" else mask.astype(f32))
    assert n == int(mask.sum())
    # a clip that is active for most rows but not all: between the norms of the live rows at a quarter
    norms = np.sort(np.linalg.norm(G[mask].astype(np.float64), axis=1))
    j = len(norms) // 4
    C = float(norms[0] / 2) if len(norms) == 1 else float((norms[j] + norms[j + 1]) / 2)
    clipped = int((norms > C).sum())
    assert clipped >= 1 and (len(norms) < 4 or clipped < len(norms))
    eloss, avg = O.combine(O.clip_rows(G, C), L)
    g = O.perturb(ks[2], avg, [K, K * d], sigma, C, n, N, f)
    # live moments on the scale of this step's gradient: b1 m_old and b2 v_old weigh as much as the new gradient's terms
    gs = np.abs(g).astype(np.float64)
    v0 = ((gs ** 2 + (0.1 * gs.max()) ** 2) * np.exp(r.uniform(-1, 1, P))).astype(f32)
    m0 = (r.normal(size=P) * np.sqrt(v0)).astype(f32)
    x, m, v = O.adam(params, m0, v0, g, i, lr=lr)

    svi = make_svi(K, d, N, C=C, sigma=sigma, lr=lr)
    st = live_state(rng.PRNGKey(seed), params, m0, v0, i, N)
    gout = torch.empty(P, device="cuda")
    new_st, loss = svi._update_gmm_fused(st, torch.tensor(X).cuda(), mask=True if mask_kind == "none" else torch.tensor(mask).cuda(),
                                         _grad_out=gout)
    what = f"K={K} d={d} B={B} mask={mask_kind} form={_form(K, d)}"
    gg = np_(gout)
    np.testing.assert_allclose(gg, g, rtol=1e-4, atol=1e-5 * np.abs(g).max(), err_msg=what)
    assert abs(float(loss) - eloss) <= 5e-5 * abs(eloss), (what, float(loss), eloss)
    assert np.array_equal(np_(new_st.rng_key).ravel(), ks[0].ravel()), what
    assert int(new_st.optim_state[0]) == i + 1
    np.testing.assert_allclose(np_(new_st.optim_state[1]), x, rtol=1e-4, atol=1e-5, err_msg=what)
    np.testing.assert_allclose(np_(new_st.optim_state[2]), m, rtol=1e-4, atol=1e-5 * np.abs(m).max(), err_msg=what)
    np.testing.assert_allclose(np_(new_st.optim_state[3]), v, rtol=1e-4, atol=1e-5 * np.abs(v).max(), err_msg=what)


# -------------------------------------------------------------------------------------------------------- D: the run loop, live
@pytest.mark.parametrize("K,d", [(16, 63), (17, 64), (3, 200)])
def test_run_steps_from_a_live_state_across_prepared_batches(rng, K, d):
    """run_steps over 65 steps (the prepared batch of 64 and one more) = 65 stepwise update() calls, bit for bit, from a live state
    at an odd step count: occupancy 3 (paired, not full), 2 (KH = 16) and 1 (DS = 4)."""
    from d3p_amd.minibatch import subsample_batchify_data
    N, B, steps, step0 = 2000, 64, 65, 11
    P = K + K * d
    r = np.random.default_rng(K * d)
    X = torch.tensor((r.normal(size=(N, d)) * 3).astype(f32)).cuda()
    params = problem(1, K, d, K + d)[1]
    v0 = (np.exp(r.uniform(-2, 2, P)) * 1e8).astype(f32)
    m0 = (r.normal(size=P) * np.sqrt(v0)).astype(f32)
    svi = make_svi(K, d, N, C=5.0, sigma=0.5, lr=1e-2)
    init, get_batch = subsample_batchify_data((X,), B)
    _, bstate = init(rng.PRNGKey(51))
    st = live_state(rng.PRNGKey(50), params, m0, v0, step0, N)
    new_st, losses = svi.run_steps(st, get_batch, bstate, 2, steps)
    ref = st
    for t in range(steps):
        ref, l = svi.update(ref, *get_batch(2 + t, bstate))
        assert float(l) == float(losses[t]), t
    assert torch.equal(ref.rng_key, new_st.rng_key) and int(new_st.optim_state[0]) == step0 + steps
    for a, b in zip(ref.optim_state[1:], new_st.optim_state[1:]):
        assert torch.equal(a, b)
    assert not torch.equal(new_st.optim_state[2], torch.tensor(m0).cuda())
