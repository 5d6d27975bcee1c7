"""The clipping diagnostics on the device (d3p_amd/clipping.py, d3p_amd/csrc/d3p_grad_norms.hip) against tests/clipping_ref.py: the
float64 autograd norms of tests/glm_ref.py with the oracle's noise streams, and a plain numpy profile.

The bound on the norms is clipping_ref.NORM_TOL: four times the float32 error of the comparator itself over the very inputs of
test_entry_against_float64, calibrated on the CPU (tests/test_clipping_host.py recomputes it); losses at glm_ref.PX_TOL."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import clipping_ref as CR
from tests import glm_ref as R

pytestmark = pytest.mark.gpu

CANARY = -7.25
PAD = 64
FAM = {"logistic": 0, "linear": 2, "poisson": 3}


def np_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def rng(gpu):
    import d3p_amd.random as r
    return r


@pytest.fixture(scope="module")
def lib(gpu):
    import d3p_amd._lib as L
    return L.load()


def model_struct(family, d, intercept, guide, N=CR.ENTRY_N, guide_code=None, fam_code=None):
    """The C struct of glm_ref.sweep_hyper: prior scales 1.5 / 2.5, lik_scale = obs_scale = N."""
    import d3p_amd._lib as L
    g = guide_code if guide_code is not None else (L.D3P_GUIDE_EXP if guide == "exp" else L.D3P_GUIDE_SOFTPLUS)
    return L.LogregModel(int(d), int(intercept), 1.5, 2.5, float(N), 1.0 / float(N), FAM[family] if fam_code is None else fam_code, g,
                         R.SWEEP_SIGMA[family] if family == "linear" else 0.0)


def padded(rows):
    buf = torch.full((rows + 2 * PAD,), CANARY, dtype=torch.float32, device="cuda")
    return buf, buf[PAD:PAD + rows]


def canaries_intact(buf, rows):
    b = np_(buf)
    return bool((b[:PAD] == CANARY).all() and (b[PAD + rows:] == CANARY).all())


def call_entry(lib, model, params, X, y, B_total, pos0, rows, eps=None, jax_key=None, want_loss=True):
    """(rc, norms, losses, canaries intact): d3p_logreg_grad_norms with canaries around both outputs."""
    import d3p_amd._lib as L
    nbuf, norms = padded(rows)
    lbuf, losses = padded(rows)
    ws = torch.empty(max(1, int(lib.d3p_logreg_grad_norms_workspace(C.byref(model), rows))), dtype=torch.uint8, device="cuda")
    rc = lib.d3p_logreg_grad_norms(L.stream_ptr(), C.byref(model), L.ptr(params), L.ptr(X), L.ptr(y), B_total, pos0, rows, L.ptr(eps),
                                   L.ptr(jax_key), L.ptr(norms), L.ptr(losses) if want_loss else None, L.ptr(ws), ws.numel())
    torch.cuda.synchronize()
    ok = canaries_intact(nbuf, rows) and canaries_intact(lbuf, rows if want_loss else 0)
    return rc, np_(norms).copy(), np_(losses).copy(), ok


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- 1. the entry against float64
@pytest.mark.parametrize("family", CR.FAMILIES)
@pytest.mark.parametrize("d", CR.ENTRY_WIDTHS)
def test_entry_against_float64(rng, lib, O, family, d):
    """{softplus, exp} x intercept {0, 1} x rows {1, 63, 65, 257} x both noise sources at this width; canaries around both outputs, X
    and the parameters unchanged, the losses within glm_ref.PX_TOL."""
    worst = 0.0
    for guide, intercept, rows, onchip, seed, X, y, loc, unc, eps in CR.entry_cases(O, family, d):
        what = f"{family} d={d} icpt={intercept} rows={rows} {guide} {'keys' if onchip else 'memory'}"
        ref, Lref, tmax = CR.norms_ref(family, CR.entry_hyper(family, d, intercept), loc, unc, X, y, eps, guide, return_t=True)
        assert tmax <= 20.0, what
        model = model_struct(family, d, intercept, guide)
        params, Xd, yd = dev(np.concatenate([loc, unc])), dev(X), dev(y)
        X0, p0 = Xd.clone(), params.clone()
        key = rng.convert_to_jax_rng_key(rng.PRNGKey(seed)).contiguous() if onchip else None
        rc, norms, losses, ok = call_entry(lib, model, params, Xd, yd, rows, 0, rows, None if onchip else dev(eps), key)
        assert rc == 0 and ok, what
        assert torch.equal(Xd, X0) and torch.equal(params, p0), what
        worst = max(worst, R.smallest_passing_rtol(norms, ref))
        tol = CR.NORM_TOL[family]
        np.testing.assert_allclose(norms, ref, rtol=tol, atol=0.1 * tol * np.abs(ref).max(), err_msg=what)
        np.testing.assert_allclose(losses, Lref, rtol=R.PX_TOL, atol=0.1 * R.PX_TOL * np.abs(Lref).max(), err_msg=what)
    print(f"{family} d={d}: worst smallest passing rtol of the norms {worst:.3e} (bound {CR.NORM_TOL[family]:.3e})")


# ---------------------------------------------------------------- 2. the entry against the device's own rows
def make_svi(family, d, intercept, N, guide="softplus", C_=1.0):
    from d3p_amd.models import (Adam, AutoDiagonalNormal, DiagonalNormalGuide, LinearRegression, LogisticRegression, MeanFieldGuide,
                                PoissonRegression, Trace_ELBO)
    from d3p_amd.svi import DPSVI
    if family == "linear":
        model = LinearRegression(d, prior_scale=1.5, intercept=intercept, intercept_prior_scale=2.5, obs_scale=R.SWEEP_SIGMA["linear"])
    elif family == "poisson":
        model = PoissonRegression(d, prior_scale=1.5, intercept=intercept, intercept_prior_scale=2.5)
    else:
        model = LogisticRegression(d, prior_scale=1.5, intercept=intercept, intercept_prior_scale=2.5)
    g = {"softplus": AutoDiagonalNormal, "exp": DiagonalNormalGuide, "sites": MeanFieldGuide}[guide](model)
    return DPSVI(model, g, Adam(1e-3), Trace_ELBO(), C_, 1.0, num_obs_total=N)


def state_with(svi, key, loc, unc, N, guide="softplus"):
    from d3p_amd.svi import DPSVIState
    d = loc.shape[0] - 1
    flat = np.concatenate([loc[d:], unc[d:], loc[:d], unc[:d]]) if guide == "sites" else np.concatenate([loc, unc])   # (tree order)
    return DPSVIState(svi.optim.init(dev(flat.astype(np.float32))), key, float(N))


def device_row_norms(svi, state, key, Xd, yd, **kw):
    """The float64 vector norm of the rows the materialising stage writes (all leaves jointly), and its losses."""
    _, px_loss, px_grads, n, f = svi._compute_per_example_gradients(state, key, Xd, yd, **kw)
    sq = sum((g.double().reshape(g.shape[0], -1) ** 2).sum(1) for g in px_grads.values())
    return np_(sq.sqrt()), np_(px_loss), px_grads


@pytest.mark.parametrize("family", CR.FAMILIES)
@pytest.mark.parametrize("d,intercept", [(4, True), (65, False), (512, True), (2048, True)])
def test_entry_against_the_devices_own_rows(rng, lib, family, d, intercept):
    """The same key and batch through d3p_logreg_px_grads: what pins the key chain inside the kernel, and pos0."""
    N, B = CR.ENTRY_N, 257
    X, y, loc, unc = R.problem(family, B, d, intercept, 31 + d, R.SWEEP_SIGMA[family])
    guide = "exp" if d in (65, 2048) else "softplus"
    svi = make_svi(family, d, intercept, N, guide)
    key = rng.PRNGKey(d + 5)
    st = state_with(svi, key, loc, unc, N)
    Xd, yd = dev(X), dev(y)
    rows_norm, rows_loss, _ = device_row_norms(svi, st, key, Xd, yd)
    model = model_struct(family, d, intercept, guide)
    jk = rng.convert_to_jax_rng_key(key).contiguous()
    rc, norms, losses, ok = call_entry(lib, model, dev(np.concatenate([loc, unc])), Xd, yd, B, 0, B, None, jk)
    assert rc == 0 and ok
    CR.check_norms(norms, rows_norm, family, f"{family} d={d} whole batch")
    np.testing.assert_allclose(losses, rows_loss, rtol=R.PX_TOL, atol=0.1 * R.PX_TOL * np.abs(rows_loss).max())
    rc, part, _, ok = call_entry(lib, model, dev(np.concatenate([loc, unc])), Xd[100:157].contiguous(), yd[100:157].contiguous(), B, 100, 57,
                                 None, jk)
    assert rc == 0 and ok
    CR.check_norms(part, rows_norm[100:157], family, f"{family} d={d} rows 100..156")


# ---------------------------------------------------------------- 3. row ranges and determinism
@pytest.mark.parametrize("family", CR.FAMILIES)
@pytest.mark.parametrize("d,intercept", [(4, True), (129, False), (2048, True)])
def test_row_ranges_and_determinism(rng, lib, family, d, intercept):
    B = 257
    X, y, loc, unc = R.problem(family, B, d, intercept, 77 + d, R.SWEEP_SIGMA[family])
    model = model_struct(family, d, intercept, "softplus")
    params, Xd, yd = dev(np.concatenate([loc, unc])), dev(X), dev(y)
    jk = rng.convert_to_jax_rng_key(rng.PRNGKey(9)).contiguous()
    rc, whole, wl, ok = call_entry(lib, model, params, Xd, yd, B, 0, B, None, jk)
    assert rc == 0 and ok
    rc, again, al, ok = call_entry(lib, model, params, Xd, yd, B, 0, B, None, jk)
    assert rc == 0 and ok and whole.tobytes() == again.tobytes() and wl.tobytes() == al.tobytes()
    rc, part, pl, ok = call_entry(lib, model, params, Xd[100:157].contiguous(), yd[100:157].contiguous(), B, 100, 57, None, jk)
    assert rc == 0 and ok and part.tobytes() == whole[100:157].tobytes() and pl.tobytes() == wl[100:157].tobytes()
    rc, _, _, ok = call_entry(lib, model, params, Xd, yd, B, 100, 0, None, jk)      # rows = 0: success, nothing written
    assert rc == 0 and ok
    rc, only, _, ok = call_entry(lib, model, params, Xd, yd, B, 0, B, None, jk, want_loss=False)     # the losses are optional
    assert rc == 0 and ok and only.tobytes() == whole.tobytes()


# ---------------------------------------------------------------- 4. non-finite rows are data
def test_poisson_row_with_infinite_rate(rng, lib):
    """exp(t) = inf (t = 96): the row's norm is not finite, of the class the materialised row's float32 norm has;
    every other row stays within the bound."""
    B, d, N = 16, 8, 16
    X, y, _, _ = R.problem("poisson", B, d, False, 21)
    loc, unc = np.ones(d, np.float32), np.full(d, -1.0, np.float32)
    Xbad = X.copy()
    Xbad[3] = 12.0
    eps = np.zeros((B, d), np.float32)
    svi = make_svi("poisson", d, False, N)
    st = state_with(svi, rng.PRNGKey(2), loc, unc, N)
    _, _, px = device_row_norms(svi, st, rng.PRNGKey(2), dev(Xbad), dev(y), _eps=dev(eps))
    G = torch.cat([px["auto_loc"], px["auto_scale"]], dim=1)
    row32 = np_((G * G).sum(1).sqrt())
    model = model_struct("poisson", d, False, "softplus", N=N)
    rc, norms, losses, ok = call_entry(lib, model, dev(np.concatenate([loc, unc])), dev(Xbad), dev(y), B, 0, B, dev(eps), None)
    assert rc == 0 and ok
    print("norm of the overflowing row:", norms[3], "materialised row:", row32[3], "loss:", losses[3])
    assert not np.isfinite(norms[3]) and np.isnan(norms[3]) == np.isnan(row32[3]) and np.isinf(norms[3]) == np.isinf(row32[3])
    keep = np.arange(B) != 3
    ref, _ = CR.norms_ref("poisson", R.hyper(d, False, 1.5, 2.5, N, N), loc, unc, X, y, eps)
    assert np.isfinite(norms[keep]).all()
    CR.check_norms(norms[keep], ref[keep], "poisson", "the other rows")


def test_linear_row_whose_squares_overflow_float32(rng, lib):
    """Finite gradient entries of ~3e19 whose squares leave float32: the norm is inf, as the float32 sum of squares of the materialised
    row is; every other row stays within the bound."""
    B, d, N = 16, 8, 10 ** 6
    X, y, loc, unc = R.problem("linear", B, d, False, 22, R.SWEEP_SIGMA["linear"])
    loc = np.ones(d, np.float32)
    Xbad = X.copy()
    Xbad[5] = 1.0e6
    eps = np.zeros((B, d), np.float32)
    from d3p_amd.svi import DPSVIState
    svi = make_svi("linear", d, False, N)
    st = DPSVIState(svi.optim.init(dev(np.concatenate([loc, unc]))), rng.PRNGKey(2), 1.0)
    _, _, px = device_row_norms(svi, st, rng.PRNGKey(2), dev(Xbad), dev(y), _eps=dev(eps))
    G = torch.cat([px["auto_loc"], px["auto_scale"]], dim=1)
    assert bool(torch.isfinite(G).all())
    row32 = np_((G * G).sum(1).sqrt())
    import d3p_amd._lib as L
    model = L.LogregModel(d, 0, 1.5, 2.5, float(N), 1.0, L.D3P_FAMILY_LINREG, L.D3P_GUIDE_SOFTPLUS, R.SWEEP_SIGMA["linear"])
    rc, norms, _, ok = call_entry(lib, model, dev(np.concatenate([loc, unc])), dev(Xbad), dev(y), B, 0, B, dev(eps), None)
    assert rc == 0 and ok
    assert np.isinf(row32[5]) and np.isinf(norms[5]) and norms[5] > 0
    keep = np.arange(B) != 5
    ref, _ = CR.norms_ref("linear", R.hyper(d, False, 1.5, 2.5, N, 1.0, R.SWEEP_SIGMA["linear"]), loc, unc, X, y, eps)
    assert np.isfinite(norms[keep]).all()
    CR.check_norms(norms[keep], ref[keep], "linear", "the other rows")


# ---------------------------------------------------------------- 5. refusals of the C entry
def test_entry_refusals(rng, lib):
    import d3p_amd._lib as L
    B, d = 8, 4
    X, y, loc, unc = R.problem("logistic", B, d, True, 3)
    params, Xd, yd = dev(np.concatenate([loc, unc])), dev(X), dev(y)
    jk = rng.convert_to_jax_rng_key(rng.PRNGKey(1)).contiguous()
    good = model_struct("logistic", d, True, "softplus")
    cases = [("Gaussian mean", L.LogregModel(d, 0, 1.5, 2.5, 1.0, 1.0, L.D3P_FAMILY_GAUSS_MEAN, 0, 0.5), params, Xd, B, 0, B),
             ("EXP_SITES", model_struct("logistic", d, True, "exp", guide_code=L.D3P_GUIDE_EXP_SITES), params, Xd, B, 0, B),
             ("pos0 + rows > B_total", good, params, Xd, B, 1, B),
             ("pos0 + rows > B_total (wraps in 32 bits)", good, params, Xd, B, 0xffffffff, 2)]
    wide = 2049
    cases.append(("d = 2049", model_struct("logistic", wide, False, "softplus"), dev(np.zeros(2 * wide, np.float32)),
                  dev(np.zeros((B, wide), np.float32)), B, 0, B))
    for what, model, p, Xc, B_total, pos0, rows in cases:
        rc, _, _, ok = call_entry(lib, model, p, Xc, yd, B_total, pos0, min(rows, B), None, jk)
        assert rc == -3, (what, rc, lib.d3p_last_error())       # D3P_E_UNSUPPORTED
        assert ok, what


# ---------------------------------------------------------------- 6. d3p_norm_profile against numpy
def raw_profile(lib, v, thr, probs):
    """The 29 words of d3p_norm_profile as (int64 array, float64 view), the positions taken over the finite count of a first call."""
    import d3p_amd._lib as L
    n = int(v.numel())
    out = torch.full((29,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(int(lib.d3p_norm_profile_workspace(n)), dtype=torch.uint8, device="cuda")
    tarr = (C.c_float * 8)(*thr)

    def call(pos):
        lo = (C.c_uint64 * 8)(*[p[0] for p in pos])
        g = (C.c_double * 8)(*[p[1] for p in pos])
        L.check(lib.d3p_norm_profile(L.stream_ptr(), L.ptr(v), n, len(thr), tarr, len(pos), lo, g, L.ptr(out), L.ptr(ws), ws.numel()))
        return np_(out).copy()
    words = call([])
    if words[0] > 0:
        words = call(CR.positions(probs, int(words[0])))
    return words, words.view(np.float64)


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("n", CR.PROFILE_SIZES)
@pytest.mark.parametrize("kind", CR.PROFILE_KINDS)
def test_norm_profile_against_numpy(lib, kind, n):
    from d3p_amd import clipping as CL
    v, thr = CR.profile_vector(kind, n)
    probs = CR.PROFILE_PROBS
    ref = CR.profile_ref(v, thr, probs)
    vd = dev(v)
    w, f = raw_profile(lib, vd, thr, probs)
    assert (int(w[0]), int(w[1])) == (ref["n_finite"], ref["n_nonfinite"])
    assert tuple(int(x) for x in w[5:13]) == ref["n_clipped"]
    assert same(float(f[4]), ref["max"])
    for q in range(8):
        got = float(f[21 + q]) if ref["n_finite"] else float("nan")
        assert same(got, ref["quantiles"][q]), (kind, n, probs[q], got, ref["quantiles"][q])
    for got, want in [(f[2], ref["mean"]), (f[3], ref["mean_sq"])] + [(f[13 + k], ref["mean_clip_factor"][k]) for k in range(8)]:
        assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= 1e-12 * abs(want), (kind, n, got, want)
    w2, _ = raw_profile(lib, vd, thr, probs)
    assert w.tobytes() == w2.tobytes()
    # the public function returns the same numbers
    p = CL.norm_profile(vd, thr, probs)
    assert (p.n, p.n_nonfinite, p.probs, p.thresholds) == (n, ref["n_nonfinite"], ref["probs"], ref["thresholds"])
    assert p.clipped_fraction == ref["clipped_fraction"]
    assert all(same(a, b) for a, b in zip(p.quantiles, ref["quantiles"])) and same(p.max, ref["max"])
    assert p.mean_clip_factor == tuple(float(x) for x in f[13:21])
    assert same(p.mean, float(f[2])) and (math.isnan(p.rms) if not ref["n_finite"] else abs(p.rms - ref["rms"]) <= 1e-12 * ref["rms"])


# ---------------------------------------------------------------- 7. the Python surface
SURFACE = [("logistic", "softplus"), ("logistic", "exp"), ("logistic", "sites"), ("linear", "softplus"), ("linear", "exp"),
           ("poisson", "softplus"), ("poisson", "exp")]


@pytest.mark.parametrize("family,guide", SURFACE)
def test_gradient_norms_equal_the_norms_of_the_materialised_rows(rng, family, guide):
    from d3p_amd import clipping as CL
    N, d = 300, 4
    X, y, loc, unc = R.problem(family, N, d, True, 55, R.SWEEP_SIGMA[family])
    svi = make_svi(family, d, True, N, guide)
    st = state_with(svi, rng.PRNGKey(12), loc, unc, N, guide)
    Xd, yd = dev(X), dev(y)
    key0, params0 = st.rng_key.clone(), st.optim_state[1].clone()
    after_plain, _ = svi.update(st, Xd, yd)
    norms, losses = CL.gradient_norms(svi, st, Xd, yd, return_losses=True)
    assert norms.shape == (N,) and norms.dtype == torch.float32 and norms.is_cuda
    default_key = rng.split(st.rng_key, 3)[1]
    want, want_loss, _ = device_row_norms(svi, st, default_key, Xd, yd)
    CR.check_norms(np_(norms), want, family, f"{family} {guide}")
    np.testing.assert_allclose(np_(losses), want_loss, rtol=R.PX_TOL, atol=0.1 * R.PX_TOL * np.abs(want_loss).max())
    assert torch.equal(CL.gradient_norms(svi, st, Xd, yd), norms)
    assert torch.equal(CL.gradient_norms(svi, st, Xd, yd, rng_key=default_key), norms)
    # the state is read, never advanced
    assert torch.equal(st.rng_key, key0) and torch.equal(st.optim_state[1], params0)
    after_call, _ = svi.update(st, Xd, yd)
    assert torch.equal(after_call.rng_key, after_plain.rng_key)
    for a, b in zip(after_call.optim_state, after_plain.optim_state):
        assert torch.equal(a, b)
    if guide == "sites":    # 20 bytes of eps per row: 100 rows per slab, three slabs
        assert torch.equal(CL.gradient_norms(svi, st, Xd, yd, slab_bytes=2000), norms)
    prof = CL.clipping_profile(svi, st, Xd, yd)
    assert prof == CL.norm_profile(norms, (1.0,), (0.5, 0.9, 0.95, 0.99))
    assert prof.thresholds == (1.0,) and prof.n == N and prof.n_nonfinite == 0


def test_python_refusals(rng):
    import d3p_amd._lib as L
    from d3p_amd import clipping as CL
    from d3p_amd.models import Adam, AutoDiagonalNormal, GaussianMean, GaussianMixtureGuide, GaussianMixtureModel, Trace_ELBO, VAEGuide, VAEModel
    from d3p_amd.svi import DPSVI
    N, d = 20, 4
    X, y, loc, unc = R.problem("logistic", N, d, True, 5)
    Xd, yd = dev(X), dev(y)
    svi = make_svi("logistic", d, True, N)
    st = state_with(svi, rng.PRNGKey(1), loc, unc, N)
    for model, guide in ((GaussianMean(d), None), (GaussianMixtureModel(k=2), GaussianMixtureGuide), (VAEModel(z_dim=2, hidden_dim=8), VAEGuide)):
        other = DPSVI(model, (guide or AutoDiagonalNormal)(model), Adam(1e-3), Trace_ELBO(), 1.0, 1.0)
        with pytest.raises(TypeError):
            CL.gradient_norms(other, st, Xd, yd)
    from d3p_amd.models import LogisticRegression
    m = LogisticRegression(d, intercept=True)
    with pytest.raises(NotImplementedError):
        CL.gradient_norms(DPSVI(m, AutoDiagonalNormal(m), Adam(1e-3), Trace_ELBO(num_particles=2), 1.0, 1.0), st, Xd, yd)
    wide = LogisticRegression(2049)
    with pytest.raises(L.D3PError, match="2048"):
        CL.gradient_norms(DPSVI(wide, AutoDiagonalNormal(wide), Adam(1e-3), Trace_ELBO(), 1.0, 1.0), st, torch.zeros(2, 2049, device="cuda"),
                          torch.zeros(2, device="cuda"))
    for kw in (dict(thresholds=(0.0,)), dict(thresholds=(float("inf"),)), dict(thresholds=tuple(range(1, 10))),
               dict(probs=tuple(i / 10 for i in range(9))), dict(probs=(1.5,))):
        with pytest.raises(ValueError):
            CL.clipping_profile(svi, st, Xd, yd, **kw)


# ---------------------------------------------------------------- 8. the profile means what it says
def test_clipped_fraction_is_the_share_of_rows_the_staged_path_rescales(rng, O):
    from d3p_amd import clipping as CL
    N, d = 257, 4
    X, y, loc, unc = R.problem("logistic", N, d, True, 91)
    key, okey = rng.PRNGKey(77), O.PRNGKey(77)
    eps = R.px_eps(O, O.convert_to_jax_rng_key(okey), N, d + 1)
    ref, _ = CR.norms_ref("logistic", R.hyper(d, True, 1.5, 2.5, N, N), loc, unc, X, y, eps)
    s = np.sort(ref)
    mid = 0.5 * (s[1:] + s[:-1])
    wide = np.nonzero((s[1:] - s[:-1]) >= 1e-3 * mid)[0]          # gap i lies between the (i+1)-th and the (i+2)-th smallest norm
    assert wide.size > 0, "no gap of relative width 1e-3 between adjacent norms"
    thresholds = []
    for point in (0.5, 0.9):
        i = wide[np.argmin(np.abs(wide - (point * (N - 1) - 0.5)))]
        thresholds.append(float(mid[i]))
    assert thresholds[0] < thresholds[1]
    Xd, yd = dev(X), dev(y)
    svi = make_svi("logistic", d, True, N)
    st = state_with(svi, key, loc, unc, N)
    prof = CL.clipping_profile(svi, st, Xd, yd, thresholds=thresholds, rng_key=key)
    for k, c in enumerate(thresholds):
        svi_c = make_svi("logistic", d, True, N, C_=c)
        _, _, px = device_row_norms(svi_c, st, key, Xd, yd)
        before = torch.cat([px["auto_loc"], px["auto_scale"]], dim=1).double().norm(dim=1)
        _, clipped = svi_c._clip_gradients(st, {k_: v.clone() for k_, v in px.items()})
        after = torch.cat([clipped["auto_loc"], clipped["auto_scale"]], dim=1).double().norm(dim=1)
        rescaled = int((after < before).sum())
        print(f"C = {c:.6g}: {rescaled} of {N} rows rescaled; clipped_fraction {prof.clipped_fraction[k]:.6f}")
        assert 0 < rescaled < N and prof.clipped_fraction[k] == rescaled / N


# ---------------------------------------------------------------- 9. the examples
def _example(name):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ex_clip_" + name, os.path.join(root, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _check_report(out):
    import re
    m = re.search(r"gradient norm quantiles 50% ([0-9.eE+-]+),", out)
    c = re.search(r"clipped fraction ([0-9.]+), mean clip factor ([0-9.]+); suggested threshold \(median norm\) ([0-9.eE+-]+)", out)
    assert m and c, out
    assert float(m.group(1)) > 0 and 0.0 <= float(c.group(1)) <= 1.0 and 0.0 <= float(c.group(2)) <= 1.0
    assert float(c.group(3)) == float(m.group(1))


@pytest.mark.parametrize("name", ["linear_regression", "poisson_regression"])
def test_regression_examples_print_a_clipping_profile(gpu, capsys, name):
    import argparse
    args = argparse.Namespace(sigma=0.5, clip_threshold=1.0, num_steps=100, learning_rate=2e-2, batch_size=100, dimensions=4,
                              num_samples=2000, obs_scale=0.5, clipping_profile=True)
    _example(name).main(args)
    _check_report(capsys.readouterr().out)


@pytest.mark.parametrize("guide", ["auto", "handwritten"])
def test_logistic_example_prints_a_clipping_profile(gpu, capsys, guide):
    import argparse
    args = argparse.Namespace(epsilon=0.1, sigma=1.0, num_epochs=1, learning_rate=1e-2, batch_size=100, dimensions=4, num_samples=2000,
                              guide=guide, predictive_accuracy=False, clipping_profile=True)
    _example("logistic_regression").main(args)
    _check_report(capsys.readouterr().out)
