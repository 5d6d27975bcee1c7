"""The stage, optimiser and mixture log-prob entries of d3p_amd/csrc/d3p_stages.hip, each called itself (the C entry through
d3p_amd._lib, not the Python wrappers) against the float64 restatements of tests/stages_ref.py, at the smallest shapes that make
every kernel loop run 0, 1 and 2 times with a ragged tail, and on the non-finite inputs the reference has a convention for.

Outputs and in-place operands are interiors of tests/workspace_harness.guarded buffers (exactly as long as the entry may write, 0xA5
guards on both sides, checked after the call); pure outputs start from the "big" or "bits" fill so that an unwritten element shows.

Bounds are in units of U = 2^-24 and count the kernel's rounded operations (docs/experiments_stages.md has the table and what the
MI355X run measured).  Every comparison prints `STAGES <entry> <case> <largest error / bound>` before it asserts.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from . import stages_ref as S
from .workspace_harness import guarded, raw_bytes

pytestmark = pytest.mark.gpu

U, TINY = S.U, S.TINY


@pytest.fixture(scope="module")
def L(gpu):
    import d3p_amd._lib as lib_module
    lib_module.load()
    return lib_module


def dev(a):
    a = np.ascontiguousarray(a)
    if a.size == 0:            # (an empty tensor has no address: one element that nothing may read stands in)
        a = np.zeros(1, a.dtype)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda().view(torch.uint32)
    return torch.from_numpy(a).cuda()


def out_buf(count, dtype=torch.float32, fill="big", seed=0):
    """A guarded pure output of `count` elements: (Guarded, typed view of its interior)."""
    g = guarded(count * torch.empty(0, dtype=dtype).element_size(), fill, "cuda", seed=seed)
    return g, g.interior.view(dtype)


def inout_buf(a):
    """A guarded in-place operand holding the numpy array `a`.  An empty one is handed over as the address of the guard behind its
    zero-byte interior, where nothing may be written."""
    a = np.ascontiguousarray(a)
    g = guarded(a.nbytes, "big", "cuda")
    dtype = torch.from_numpy(a).dtype
    if not a.nbytes:
        return g, g.raw[g.offset:g.offset + 4].view(dtype)
    g.interior.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
    return g, g.interior.view(dtype)


def host(t):
    return t.detach().cpu().numpy()


def within(entry, case, got, ref, bound):
    """|got - ref| <= bound elementwise where ref is finite; NaN and +-inf must be met exactly; a zero bound means equality."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    bound = np.broadcast_to(np.asarray(bound, np.float64).reshape(-1) if np.ndim(bound) else bound, ref.shape)
    assert got.shape == ref.shape, (entry, case, got.shape, ref.shape)
    nan, inf = np.isnan(ref), np.isinf(ref)
    assert np.array_equal(np.isnan(got), nan), (entry, case, "NaN pattern", np.flatnonzero(np.isnan(got) != nan)[:8])
    assert np.array_equal(got[inf], ref[inf]), (entry, case, "infinities")
    fin = ~(nan | inf)
    err, b = np.abs(got[fin] - ref[fin]), bound[fin]
    with np.errstate(all="ignore"):
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"STAGES {entry} {case} {worst:.4f}")
    assert worst <= 1.0, (entry, case, worst, int(np.flatnonzero(fin)[int(ratio.argmax())]))
    return worst


# ------------------------------------------------------------------------------------------------------------ d3p_clip_rows
@pytest.mark.parametrize("case_index", range(len(S.clip_cases())))
def test_clip_rows(L, case_index):
    """|got - ref| <= (ceil(P / 64) + 16) U |ref| per element: a lane's chain of ceil(P / 64) fmas of non-negative terms, the six
    adds of the wave sum, the root, two divisions, the multiply, and slack for the wave sum's order.  Rows of the seven kinds of
    stages_ref.CLIP_KINDS rotate through the row positions: a NaN row is NaN throughout, a row whose float32 sum of squares
    overflows is 0 (an infinite entry: NaN there), and their neighbours are what they are without them."""
    P, B = S.clip_cases()[case_index]
    g, c = S.clip_input(case_index)
    ref, mag = S.clip_rows(g, c)
    buf, view = inout_buf(g)
    L.check(L.load().d3p_clip_rows(L.stream_ptr(), L.ptr(view), B, P, c))
    got = host(view).reshape(B, P)
    buf.check("d3p_clip_rows")
    within("clip_rows", f"P={P},B={B}", got, ref, (-(-P // 64) + 16) * U * mag)
    for r in range(B):
        kind = S.clip_kind(case_index, r)
        if kind == "nan":
            assert np.isnan(got[r]).all()
        elif kind == "overflow":
            assert (got[r] == 0).all()
        elif kind == "below":
            assert np.array_equal(got[r], g[r])          # scale 1: the row's own bits
        elif kind == "above":
            assert math.sqrt((got[r].astype(np.float64) ** 2).sum()) <= c * (1 + (-(-P // 64) + 16) * U)


def test_clip_rows_infinite_threshold_is_the_identity_and_zero_is_refused(L):
    g, _ = S.clip_input(9)
    keep = [r for r in range(g.shape[0]) if S.clip_kind(9, r) in ("below", "above", "at_c", "zero")]
    g = np.ascontiguousarray(g[keep])
    assert g.shape[0] >= 2
    buf, view = inout_buf(g)
    L.check(L.load().d3p_clip_rows(L.stream_ptr(), L.ptr(view), g.shape[0], g.shape[1], math.inf))
    assert np.array_equal(raw_bytes(view).numpy(), g.reshape(-1).view(np.uint8))
    with pytest.raises(ValueError, match="clipping threshold"):
        L.check(L.load().d3p_clip_rows(L.stream_ptr(), L.ptr(view), g.shape[0], g.shape[1], 0.0))
    torch.cuda.synchronize()
    assert np.array_equal(raw_bytes(view).numpy(), g.reshape(-1).view(np.uint8))
    buf.check("d3p_clip_rows")


# ------------------------------------------------------------------------------------------------------------ d3p_full_norm(_ord)
@pytest.mark.parametrize("n,content", S.norm_cases())
def test_full_norm_every_order(L, n, content):
    """numpy.linalg.norm in float64 for the eight orders: counts and selections exactly (a NaN at index 0, 255, 256 or n - 1 gives
    what numpy gives, +-inf entries too; at ord = -inf the idle threads' +inf never wins), sums within stages_ref.norm_bound."""
    lib = L.load()
    for k, v in enumerate(S.norm_inputs(n, content)):
        v_dev = dev(v)
        for order in S.NORM_ORDS:
            ref, _ = S.full_norm(v, order)
            buf, out = out_buf(1, seed=k)
            L.check(lib.d3p_full_norm_ord(L.stream_ptr(), L.ptr(v_dev), n, float(order), L.ptr(out)))
            got = host(out)
            buf.check("d3p_full_norm_ord")
            within(f"full_norm_ord[{order}]", f"n={n},{content}#{k}", got, [ref], S.norm_bound(n, order) * abs(ref))
            if order == -math.inf and content in ("mixed", "equal", "zeros"):
                assert np.isfinite(got[0])
        ref, _ = S.full_norm(v, 2)
        buf, out = out_buf(1, fill="bits", seed=k)
        L.check(lib.d3p_full_norm(L.stream_ptr(), L.ptr(v_dev), n, L.ptr(out), None, 0))
        got = host(out)
        buf.check("d3p_full_norm")
        within("full_norm", f"n={n},{content}#{k}", got, [ref], S.norm_bound(n, 2) * abs(ref))


def test_full_norm_of_nothing_is_zero(L):
    buf, out = out_buf(1)
    L.check(L.load().d3p_full_norm(L.stream_ptr(), None, 0, L.ptr(out), None, 0))
    assert raw_bytes(out).tolist() == [0, 0, 0, 0]
    buf.check("d3p_full_norm")
    with pytest.raises(ValueError):
        L.check(L.load().d3p_full_norm_ord(L.stream_ptr(), None, 0, 1.0, L.ptr(out)))


# ------------------------------------------------------------------------------------------------------------ d3p_combine
@pytest.mark.parametrize("B,P", S.combine_cases())
def test_combine(L, B, P):
    """Column means within (ceil(B / 8) + 10) U sum|g| / B (a row group's chain of ceil(B / 8) adds, eight adds across the groups,
    the division), the mean loss within (ceil(B / 256) + 10) U sum|l| / B; columns that cancel to 2^-12 of their terms; without the
    loss pair nothing is written there; a NaN makes its column NaN and leaves every other column's bits."""
    lib = L.load()
    g, loss = S.combine_input(B, P)
    avg_ref, avg_cond, loss_ref, loss_cond = S.combine(g, loss)
    g_dev, loss_dev = dev(g), dev(loss)
    abuf, avg = out_buf(P)
    lbuf, lout = out_buf(1, fill="bits")
    L.check(lib.d3p_combine(L.stream_ptr(), L.ptr(g_dev), L.ptr(loss_dev), B, P, L.ptr(avg), L.ptr(lout)))
    clean = host(avg).copy()
    within("combine", f"B={B},P={P}", clean, avg_ref, (-(-B // 8) + 10) * U * avg_cond)
    within("combine.loss", f"B={B},P={P}", host(lout), [loss_ref], (-(-B // 256) + 10) * U * loss_cond)
    abuf.check("d3p_combine avg")
    lbuf.check("d3p_combine loss")
    # one NaN, no loss pair
    col, row = (P * 2) // 3, B // 2
    g2 = g.copy()
    g2[row, col] = np.nan
    abuf, avg = out_buf(P, fill="bits")
    lbuf, lout = out_buf(1, fill="bits", seed=1)
    before = raw_bytes(lout).clone()
    g2_dev = dev(g2)
    L.check(lib.d3p_combine(L.stream_ptr(), L.ptr(g2_dev), None, B, P, L.ptr(avg), L.ptr(lout)))
    got = host(avg)
    abuf.check("d3p_combine avg")
    assert torch.equal(raw_bytes(lout), before)
    assert np.isnan(got[col])
    others = np.arange(P) != col
    assert np.array_equal(got[others].view(np.uint32), clean[others].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ d3p_perturb
@pytest.mark.parametrize("sizes", S.PERTURB_SITES, ids=lambda s: "x".join(map(str, s)))
def test_perturb_sites(L, O, sizes):
    """Against the oracle's perturb at tests/test_gpu_dpsvi.py's tolerance: a zero-size site consumes its key and writes nothing,
    and the last ChaCha block of a site is partial, so the guard directly behind the last element must be intact."""
    total = sum(sizes)
    dp_scale, c, n, obs_scale, factor = 1.3, 0.8, 48.0, 0.3, 64.0 / 48.0
    avg = S.f32(np.linspace(-1.0, 1.0, total) if total > 1 else np.array([0.25]))
    key = O.PRNGKey(97 + len(sizes))
    want = O.perturb(key, avg, sizes, dp_scale, c, n, obs_scale, factor)
    obuf, out = out_buf(total, fill="bits")
    kbuf, keys = out_buf(16 * len(sizes), dtype=torch.int32, fill="bits", seed=2)
    meta = dev(S.f32([n, np.float32(factor)]))
    arr = (C.c_int32 * len(sizes))(*sizes)
    key_d, avg_d = dev(np.asarray(key, np.uint32).reshape(-1)), dev(avg)
    L.check(L.load().d3p_perturb(L.stream_ptr(), L.ptr(key_d), L.ptr(avg_d), arr, len(sizes), dp_scale, c,
                                 L.ptr(meta), obs_scale, L.ptr(out), L.ptr(keys)))
    got = host(out)
    obuf.check("d3p_perturb out")
    kbuf.check("d3p_perturb site keys")
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)
    assert np.array_equal(host(keys).view(np.uint32).reshape(len(sizes), 16), O.split(key, len(sizes)).reshape(len(sizes), 16))


@pytest.mark.parametrize("n", S.APPLY_N)
def test_perturb_apply(L, n):
    """(avg + noise * dp_scale * c / n) * obs_scale * factor within 3 U (|avg| + |noise scale|) |obs_scale factor|."""
    rng = np.random.default_rng([707, n])
    avg, noise = S.f32(rng.standard_normal(n) * 0.2), S.f32(rng.standard_normal(n))
    dp_scale, c, num, obs_scale, factor = 1.3, 0.8, 48.0, 0.3, float(np.float32(64.0 / 48.0))
    ref, cond = S.perturb_apply(avg, noise, dp_scale, c, num, obs_scale, factor)
    obuf, out = out_buf(n)
    avg_d, noise_d, meta = dev(avg), dev(noise), dev(S.f32([num, factor]))
    L.check(L.load().d3p_perturb_apply(L.stream_ptr(), L.ptr(avg_d), L.ptr(noise_d), n, dp_scale, c, L.ptr(meta), obs_scale, L.ptr(out)))
    got = host(out)
    obuf.check("d3p_perturb_apply")
    within("perturb_apply", f"n={n}", got, ref, 3 * U * cond)


# ------------------------------------------------------------------------------------------------------------ d3p_adam_step, d3p_sgd_step
@pytest.mark.parametrize("P,i", S.adam_cases())
def test_adam_step(L, P, i):
    """x, m and v of one step at counter i, from zero and from random moments, at numpyro's defaults and one other set of
    hyperparameters.  m and v within 4 U of their terms' magnitudes (+ 2^-126: a denormal g^2 may flush); x within
    U |x| + (24 U + e_i a_i) |update| + 4 U |update with m's terms in the place of m|, where a_i is how an error of b^(i+1)
    reaches the update and e_i that error (stages_ref.adam_pow_eps); the last term is m's own error, which is relative to its two
    terms and not to their sum: from random moments (1 - b1) g and b1 m cancel to 1 / 500 of themselves in some element, and a
    float32 numpy evaluation of the formula is as far from float64 there as the kernel.  g = 1e20: g * g is +inf, so v = +inf and x keeps its bits.  The counter is i + 1, also at P = 0."""
    lib = L.load()
    for h, hyper in enumerate(S.ADAM_HYPER):
        for random_moments in (False, True):
            x, m, v, g, special = S.adam_input(P, i, random_moments)
            ref = S.adam(x, m, v, g, i, *hyper)
            xb, xv = inout_buf(x)
            mb, mv = inout_buf(m)
            vb, vv = inout_buf(v)
            sb, step = inout_buf(np.array([i], np.int32))
            g_d = dev(g)
            L.check(lib.d3p_adam_step(L.stream_ptr(), L.ptr(xv), L.ptr(mv), L.ptr(vv), L.ptr(step), L.ptr(g_d), P, *hyper))
            gx, gm, gv = host(xv)[:P], host(mv)[:P], host(vv)[:P]
            assert int(step.item()) == i + 1
            for b in (xb, mb, vb, sb):
                b.check("d3p_adam_step")
            case = f"P={P},i={i},h={h},m={int(random_moments)}"
            within("adam.m", case, gm, ref["m"], 4 * U * ref["cond_m"] + TINY)
            within("adam.v", case, gv, ref["v"], 4 * U * np.where(np.isfinite(ref["cond_v"]), ref["cond_v"], 0.0) + TINY)
            amp = S.adam_power_amplification(i, hyper[1], hyper[2])
            within("adam.x", case, gx, ref["x"], U * np.abs(x.astype(np.float64)) + (24 * U + S.adam_pow_eps(i) * amp) * ref["upd"]
                   + 4 * U * np.where(np.isfinite(ref["upd_cond"]), ref["upd_cond"], 0.0) + TINY)
            big = special == 3
            assert np.isposinf(gv[big]).all() and np.array_equal(gx[big].view(np.uint32), x[big].view(np.uint32))
            assert np.isfinite(gv[~big]).all() and np.isfinite(gx).all() and np.isfinite(gm).all()


@pytest.mark.parametrize("P", S.ADAM_P)
def test_sgd_step(L, P):
    """x - lr g within 2 U (|x| + |lr g|); the counter increments, also at P = 0."""
    rng = np.random.default_rng([808, P])
    x, g, lr = S.f32(rng.standard_normal(P)), S.f32(rng.standard_normal(P) * 3.0), 0.37
    ref, cond = S.sgd(x, g, lr)
    xb, xv = inout_buf(x)
    sb, step = inout_buf(np.array([41], np.int32))
    g_d = dev(g)
    L.check(L.load().d3p_sgd_step(L.stream_ptr(), L.ptr(xv), L.ptr(step), L.ptr(g_d), P, lr))
    got = host(xv)[:P]
    assert int(step.item()) == 42
    xb.check("d3p_sgd_step")
    sb.check("d3p_sgd_step")
    within("sgd", f"P={P}", got, ref, 2 * U * cond)


# ------------------------------------------------------------------------------------------------------------ d3p_adadp_step
def _adadp_state(L, x0):
    P = x0.size
    bufs = {"x": inout_buf(x0), "x_stepped": out_buf(P), "x_prev": out_buf(P, fill="bits"),
            "lr": inout_buf(np.array([S.ADADP_LR0], np.float32)), "step": inout_buf(np.array([0], np.int32))}
    nbytes = int(L.load().d3p_adadp_workspace())
    assert nbytes == 65 * 4                       # 64 partial sums and the next learning rate: the whole workspace
    bufs["ws"] = (guarded(nbytes, "bits", "cuda", seed=P), None)
    return bufs


def _adadp_call(L, bufs, g, P, tol, check, ws_bytes=None):
    ws, g_d = bufs["ws"][0], dev(g)
    L.check(L.load().d3p_adadp_step(L.stream_ptr(), L.ptr(bufs["x"][1]), L.ptr(bufs["lr"][1]), L.ptr(bufs["x_stepped"][1]),
                                    L.ptr(bufs["x_prev"][1]), L.ptr(bufs["step"][1]), L.ptr(g_d), P, tol, int(check),
                                    L.ptr(ws.interior), ws.nbytes if ws_bytes is None else ws_bytes))
    state = {k: host(bufs[k][1]).copy() for k in ("x", "x_stepped", "x_prev", "lr", "step")}
    for k, (b, _) in bufs.items():
        b.check(f"d3p_adadp_step {k}")
    return state


@pytest.mark.parametrize("P,scenario", S.adadp_cases())
def test_adadp_step(L, P, scenario):
    """An even step, then an odd one.  x, x_prev and x_stepped within 2 U (|x| + |lr g|) after each; the learning rate is kept by
    the even step and within (ceil(P / 16384) + 64 + 16) U of lr sqrt(tol / err) after the odd one (the clamps 0.9 / 1.1 exactly);
    a rejected step leaves x_prev's bits in x; the counter counts."""
    x0, g0, g1, tol, check = S.adadp_input(P, scenario)
    bufs = _adadp_state(L, x0)
    case = f"P={P},{scenario}"
    ref = S.adadp(x0, S.ADADP_LR0, S.f32(np.zeros(P)), x0, g0, 0, tol, check)
    st = _adadp_call(L, bufs, g0, P, tol, check)
    assert st["step"][0] == 1 and st["lr"][0] == np.float32(S.ADADP_LR0)
    for name in ("x", "x_stepped", "x_prev"):
        within(f"adadp.{name}", case + ",even", st[name], ref[name], 2 * U * ref["cond"])
    assert np.array_equal(st["x_prev"].view(np.uint32), x0.view(np.uint32))
    ref = S.adadp(st["x"], st["lr"][0], st["x_stepped"], st["x_prev"], g1, 1, tol, check)
    st2 = _adadp_call(L, bufs, g1, P, tol, check)
    assert st2["step"][0] == 2
    for name in ("x", "x_stepped", "x_prev"):
        within(f"adadp.{name}", case + ",odd", st2[name], ref[name], 2 * U * ref["cond"])
    assert ref["reject"] == (scenario == "reject")
    if scenario == "reject":
        assert np.array_equal(st2["x"].view(np.uint32), st["x_prev"].view(np.uint32))
    if scenario == "zero_grad":
        assert st2["lr"][0] == np.float32(st["lr"][0]) * np.float32(1.1)
    else:
        within("adadp.lr", case, st2["lr"], [ref["lr"]], S.adadp_lr_bound(P) * ref["lr"])
        assert 0.9 * st["lr"][0] < st2["lr"][0] < 1.1 * st["lr"][0]


def test_adadp_refuses_a_short_workspace_before_any_launch(L):
    x0, g0, _, tol, check = S.adadp_input(257, "accept")
    bufs = _adadp_state(L, x0)
    before = {k: raw_bytes(b.interior).clone() for k, (b, _) in bufs.items()}
    with pytest.raises(L.D3PError, match="workspace"):
        _adadp_call(L, bufs, g0, 257, tol, check, ws_bytes=65 * 4 - 1)
    torch.cuda.synchronize()
    for k, (b, _) in bufs.items():
        assert torch.equal(raw_bytes(b.interior), before[k]), k
        b.check(k)


# ------------------------------------------------------------------------------------------------------------ d3p_gmm_log_prob
def _gmm_call(L, x, locs, scales, pis, fill="big"):
    B, d = x.shape
    buf, out = out_buf(B, fill=fill)
    x_d, locs_d, scales_d, pis_d = dev(x), dev(locs), dev(scales), dev(pis)
    L.check(L.load().d3p_gmm_log_prob(L.stream_ptr(), L.ptr(x_d), B, d, L.ptr(locs_d), L.ptr(scales_d), L.ptr(pis_d),
                                      locs.shape[0], L.ptr(out)))
    got = host(out).copy()
    buf.check("d3p_gmm_log_prob")
    return got


@pytest.mark.parametrize("K,d,B", S.gmm_cases())
def test_gmm_log_prob(L, K, d, B):
    """Finite rows at tests/test_gpu_gmm.py's tolerance against the float64 restatement, with one pi = 0 and a component 10^3
    log-units away.  Hostile rows -- an infinite coordinate, a finite row at 1e30 (z * z beyond float32): -inf, as jax's logsumexp
    gives when every component is -inf; a NaN coordinate: NaN -- placed first, inside a 4-row workgroup and last, exactly; their
    neighbours keep the bits they have without them."""
    x, locs, scales, pis = S.gmm_input(K, d, B)
    clean = _gmm_call(L, x, locs, scales, pis)
    ref, _ = S.gmm_log_prob(x, locs, scales, pis)
    within("gmm_log_prob", f"K={K},d={d},B={B}", clean, ref, S.GMM_RTOL * np.abs(ref) + S.GMM_ATOL)
    for rotation in range(3):
        xh, placed = S.gmm_hostile(x, rotation)
        got = _gmm_call(L, xh, locs, scales, pis, fill="bits")
        want, _ = S.gmm_log_prob(xh, locs, scales, pis)
        for row, kind in placed.items():
            assert np.array_equal(got[row], np.float32(want[row]), equal_nan=True), (kind, row, got[row], want[row])
            assert np.isnan(got[row]) if kind == "nan" else got[row] == -np.inf
        keep = np.array([r not in placed for r in range(B)])
        assert np.array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32))


def test_gmm_log_prob_refuses_k_beyond_64_and_k_zero_before_any_launch(L):
    x, locs, scales, pis = S.gmm_input(4, 3, 5)
    buf, out = out_buf(5, fill="bits")
    before = raw_bytes(out).clone()
    held = [dev(a) for a in (x, locs, scales, pis)]
    args = (L.stream_ptr(), L.ptr(held[0]), 5, 3, L.ptr(held[1]), L.ptr(held[2]), L.ptr(held[3]))
    with pytest.raises(L.D3PError, match="at most 64 mixture components"):
        L.check(L.load().d3p_gmm_log_prob(*args, 65, L.ptr(out)))
    with pytest.raises(ValueError, match="d and K must be >= 1"):
        L.check(L.load().d3p_gmm_log_prob(*args, 0, L.ptr(out)))
    torch.cuda.synchronize()
    assert torch.equal(raw_bytes(out), before)
    buf.check("d3p_gmm_log_prob")


def test_gaussian_mixture_log_prob_keeps_a_minus_inf_row_through_its_reshape(gpu):
    from d3p_amd.gmm import GaussianMixture
    x, locs, scales, pis = S.gmm_input(5, 7, 6)
    x[4, 3] = np.inf
    got = host(GaussianMixture(locs, scales, pis).log_prob(torch.tensor(x.reshape(2, 3, 7))))
    ref = S.gmm_log_prob(x, locs, scales, pis)[0].reshape(2, 3)
    assert got.shape == (2, 3) and got[1, 1] == -np.inf and ref[1, 1] == -np.inf
    fin = np.isfinite(ref)
    assert fin.sum() == 5 and np.allclose(got[fin], ref[fin], rtol=S.GMM_RTOL, atol=S.GMM_ATOL)
    assert float(GaussianMixture(locs, scales, pis).log_prob(torch.tensor(x[4]))) == -np.inf


# ------------------------------------------------------------------------------------------------------------ d3p_tf_randint
@pytest.mark.parametrize("lo,hi", S.RANDINT_RANGES)
@pytest.mark.parametrize("n", S.RANDINT_N)
def test_tf_randint(L, O, n, lo, hi):
    """Bit for bit against the oracle and against the Python-integer restatement of jax's combination, fed the oracle's split keys
    and word streams: spans up to 2^32 - 1, where the wrapping 32-bit multiplier is not 2^32 % span."""
    key = np.array([11, 500 + n], np.uint32)
    buf, out = out_buf(n, dtype=torch.int32, fill="bits")
    key_d = dev(key)
    L.check(L.load().d3p_tf_randint(L.stream_ptr(), L.ptr(key_d), n, lo, hi, L.ptr(out)))
    got = host(out)
    buf.check("d3p_tf_randint")
    assert np.array_equal(got, O.tf_randint(key, n, lo, hi))
    k = O.tf_split(key, 2)
    assert np.array_equal(got, S.tf_randint(O.tf_random_words(k[0], n), O.tf_random_words(k[1], n), lo, hi))
    assert got.min() >= lo and got.max() <= max(hi - 1, lo)
