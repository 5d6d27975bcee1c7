"""d3p_amd.mixture_diagnostics on the GPU: d3p_gmm_loglik_draw_sums against the float64 row sums of THE
DEVICE'S OWN rows-form matrix (d3p_gmm_loglik_rows, pinned by tests/mixture_density_ref.py: only the new summation is judged) within
the float64 reordering bound rows 2^-53 sum_r |ll[s, r]| -- derived, not measured -- and, bit for bit, against the stated summation
order applied to that matrix (tests/mixture_diag_ref.tree_totals); strips, determinism, special values, extents and refusals;
log_likelihood_total, log_joint and guide_diagnostic against tests/mixture_diag_ref.py on the device's own draws; the example's flag."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import guide_diag_ref as G
from tests import mixture_density_ref as D
from tests import mixture_diag_ref as R
from tests import predictive_ref as P
from tests import psis_ref as PR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 12345.0
KS = (1, 3, 4, 5, 16, 17, 32)
DS = (1, 2, 63, 64, 65, 128, 256)
ROWS = (1, 63, 64, 65, 129)
NS = (1, 3, 4, 5, 9)
# (k, d, rows, n): every value of the four axes at least once; the three KMAX instantiations (4 / 16 / 32) at their edges; both shapes
# whose draws are split over two waves, (16, 256) and (32, 128), with an odd number of draws (a wave idles in the last pass)
SWEEP = [(1, 63, 1, 1), (3, 2, 63, 3), (4, 65, 64, 4), (5, 1, 65, 5), (16, 256, 129, 9), (17, 64, 64, 3), (32, 128, 129, 5),
         (3, 2, 129, 9), (16, 64, 65, 4)]


def np_(t):
    return t.detach().cpu().numpy()


def _mg(**kw):
    from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel
    m = GaussianMixtureModel(**kw)
    return m, GaussianMixtureGuide(m)


@pytest.fixture(scope="module")
def MDG(gpu):
    from d3p_amd import mixture_diagnostics
    return mixture_diagnostics


def test_the_sweep_covers_every_axis_value():
    assert {c[0] for c in SWEEP} == set(KS) and {c[1] for c in SWEEP} == set(DS)
    assert {c[2] for c in SWEEP} == set(ROWS) and {c[3] for c in SWEEP} == set(NS)
    assert all(D.draw_waves(k, d) == (2 if (k, d) in ((16, 256), (32, 128)) else 4) for k, d, _, _ in SWEEP)
    assert {(16, 256), (32, 128)} <= {(c[0], c[1]) for c in SWEEP}


# ---------------------------------------------------------------- the entry against its comparator
def pack(pis, mus, sigs, extra=3):
    """The latent buffer at a leading dimension `extra` above the row's length, canaries in the padding: (tensor, ld)."""
    n, k = pis.shape
    kd = mus.reshape(n, -1).shape[1]
    ld = k + 2 * kd + extra
    lat = torch.full((n, ld), CANARY, device="cuda")
    lat[:, :k] = torch.tensor(np.array(pis)).cuda()
    lat[:, k:k + kd] = torch.tensor(np.array(mus)).cuda().reshape(n, kd)
    lat[:, k + kd:k + 2 * kd] = torch.tensor(np.array(sigs)).cuda().reshape(n, kd)
    return lat, ld


def rows_matrix(x, lat, ld, k, n):
    """The device's own (n, rows) float32 matrix from the same latent buffer, as numpy."""
    import d3p_amd._lib as L
    rows, d = x.shape
    ll = torch.empty((n, rows), device="cuda")
    L.check(L.load().d3p_gmm_loglik_rows(L.stream_ptr(), L.ptr(x), rows, d, L.ptr(lat), ld, k, n, L.ptr(ll)))
    return np_(ll)


def draw_sums_entry(x, lat, ld, k, n, pad=16):
    """d3p_gmm_loglik_draw_sums with canaries on both sides of the output and of the workspace: (n,) float64 numpy after the canaries
    and the inputs were checked."""
    import d3p_amd._lib as L
    lib = L.load()
    rows, d = x.shape
    before = lat.clone()
    nbytes = lib.d3p_gmm_loglik_draw_sums_workspace(rows, d, k, n)
    assert nbytes == 8 * R.strips_of(rows)[0] * n
    out = torch.full((n + 2 * pad,), CANARY, dtype=torch.float64, device="cuda")
    ws = torch.full((nbytes // 8 + 2 * pad,), CANARY, dtype=torch.float64, device="cuda")
    L.check(lib.d3p_gmm_loglik_draw_sums(L.stream_ptr(), L.ptr(x), rows, d, L.ptr(lat), ld, k, n, L.ptr(out[pad:]), L.ptr(ws[pad:]), nbytes))
    torch.cuda.synchronize()
    assert bool((out[:pad] == CANARY).all()) and bool((out[pad + n:] == CANARY).all()), "the output was written outside its extent"
    assert bool((ws[:pad] == CANARY).all()) and bool((ws[pad + nbytes // 8:] == CANARY).all()), "the workspace was written outside its extent"
    assert torch.equal(lat.view(torch.int32), before.view(torch.int32))      # (bits: a planted NaN stays where it was)
    return np_(out[pad:pad + n]).copy()


def assert_sums(got, ll, what):
    """got (n,) float64 against the float64 row sums of ll (n, rows) float32 within rows 2^-53 sum |ll|; draws whose sum is not
    finite agree exactly; and the stated summation order on the same matrix gives the same BITS."""
    ref, bound = G.totals(ll), G.totals_bound(ll)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), what + ": the non-finite draws differ"
    err = np.abs(got[fin] - ref[fin])
    if fin.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"{what}: largest error / bound {np.nanmax(np.where(bound[fin] > 0, err / bound[fin], 0.0)):.3f}, "
                  f"largest relative error {np.max(err / np.maximum(np.abs(ref[fin]), 1e-300)):.2e}")
    assert np.all(err <= bound[fin]), f"{what}: error {err.max():.3e} above the bound"
    tree = R.tree_totals(ll)
    assert np.array_equal(got[fin].view(np.int64), tree[fin].view(np.int64)), what + ": not the stated order on the rows form's values"


def _case(k, d, rows, n):
    obs, pis, mus, sigs = D.soft_inputs(k, d, rows, n)
    x = torch.tensor(obs).cuda()
    lat, ld = pack(pis, mus, sigs)
    return x, lat, ld


@pytest.mark.parametrize("k,d,rows,n", SWEEP)
def test_draw_sums_at_every_edge(gpu, k, d, rows, n):
    x, lat, ld = _case(k, d, rows, n)
    ll = rows_matrix(x, lat, ld, k, n)
    assert ll.shape == (n, rows) and np.isfinite(ll).all()
    assert_sums(draw_sums_entry(x, lat, ld, k, n), ll, f"k={k} d={d} rows={rows} n={n}")


@pytest.mark.parametrize("k,d,rows,n,what", [
    (3, 2, 7000 * 64 + 5, 5, "four tiles per strip, a ragged last tile"),     # tiles = 7001: per = 4, 1751 strips, the last of 1 tile of 5 rows
    (3, 2, 2048 * 64 - 37, 3, "the largest strip count"),                     # tiles = 2048 = strips, the last ragged
    (5, 7, 200, 9, "four strips of one tile"),
])
def test_draw_sums_over_strips(gpu, k, d, rows, n, what):
    strips, per = R.strips_of(rows)
    assert {"four tiles per strip, a ragged last tile": per == 4 and strips == 1751 and rows % 64 == 5,
            "the largest strip count": strips == 2048 and per == 1 and rows % 64, "four strips of one tile": strips == 4 and rows % 64}[what]
    x, lat, ld = _case(k, d, rows, n)
    ll = rows_matrix(x, lat, ld, k, n)
    got = draw_sums_entry(x, lat, ld, k, n)
    assert_sums(got, ll, what)
    again = draw_sums_entry(x, lat, ld, k, n)
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), "two calls differ"


def test_draw_sums_do_not_depend_on_the_other_draws(gpu):
    """The same table with draws appended: the first n sums keep their bits (9 draws against their first 5 and first 1)."""
    k, d, rows = 5, 7, 200
    obs, pis, mus, sigs = D.soft_inputs(k, d, rows, 9)
    x = torch.tensor(obs).cuda()
    whole = draw_sums_entry(x, *pack(pis, mus, sigs), k, 9)
    for n in (5, 1):
        part = draw_sums_entry(x, *pack(pis[:n], mus[:n], sigs[:n]), k, n)
        assert np.array_equal(whole[:n].view(np.int64), part.view(np.int64)), n


# ---------------------------------------------------------------- special values
def test_special_values_stay_with_their_draw(gpu):
    k, d, rows, n = 3, 5, 131, 6
    obs, pis, mus, sigs = (np.array(v) for v in D.soft_inputs(k, d, rows, n))
    x = torch.tensor(obs).cuda()
    p = pis.copy()
    p[2] = 0.0                                                # every weight of draw 2 zero: ll = -inf in every row
    lat, ld = pack(p, mus, sigs)
    ll = rows_matrix(x, lat, ld, k, n)
    assert np.isneginf(ll[2]).all() and np.isfinite(np.delete(ll, 2, axis=0)).all()
    got = draw_sums_entry(x, lat, ld, k, n)
    assert got[2] == -np.inf and np.isfinite(np.delete(got, 2)).all()
    assert_sums(got, ll, "one draw of zero weights")
    m = mus.copy()
    m[4, 1, 3] = np.nan                                       # a NaN in one draw's latents: that draw only
    lat, ld = pack(pis, m, sigs)
    got = draw_sums_entry(x, lat, ld, k, n)
    assert np.isnan(got[4]) and np.isfinite(np.delete(got, 4)).all()
    xn = obs.copy()
    xn[70, 2] = np.nan                                        # a NaN in a row of obs: every draw
    lat, ld = pack(pis, mus, sigs)
    assert np.isnan(draw_sums_entry(torch.tensor(xn).cuda(), lat, ld, k, n)).all()


def test_no_rows_give_zeros_without_a_launch(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    x, lat = torch.zeros((1, 2), device="cuda"), torch.ones((5, 15), device="cuda")
    out = torch.full((9,), CANARY, dtype=torch.float64, device="cuda")
    assert lib.d3p_gmm_loglik_draw_sums_workspace(0, 2, 3, 5) == 0
    assert lib.d3p_gmm_loglik_draw_sums(L.stream_ptr(), L.ptr(x), 0, 2, L.ptr(lat), 15, 3, 5, L.ptr(out[2:]), None, 0) == 0
    torch.cuda.synchronize()
    assert bool((out[2:7] == 0.0).all()) and bool((out[:2] == CANARY).all()) and bool((out[7:] == CANARY).all())


def test_c_entry_refuses_before_any_launch(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    UNSUPPORTED, INVALID = -3, -1
    k, d, rows, n = 3, 2, 40, 6
    x = torch.zeros((rows, d), device="cuda")
    lat = torch.ones((n, 15), device="cuda")
    lat[:, :k] = 1.0 / k
    out = torch.full((n + 2,), CANARY, dtype=torch.float64, device="cuda")
    ws = torch.full((n + 2,), CANARY, dtype=torch.float64, device="cuda")
    nbytes = lib.d3p_gmm_loglik_draw_sums_workspace(rows, d, k, n)
    assert nbytes == 8 * n

    def run(x_=L.ptr(x), rows_=rows, d_=d, lat_=L.ptr(lat), ld=15, k_=k, n_=n, out_=L.ptr(out[1:]), ws_=L.ptr(ws[1:]), bytes_=nbytes):
        return lib.d3p_gmm_loglik_draw_sums(L.stream_ptr(), x_, rows_, d_, lat_, ld, k_, n_, out_, ws_, bytes_)
    assert run(x_=None) == INVALID and run(lat_=None) == INVALID and run(out_=None) == INVALID
    odd = C.c_void_p(x.data_ptr() + 2)
    assert run(x_=odd) == INVALID and b"aligned to 4" in lib.d3p_last_error()
    for kk, dd in ((0, 2), (2, 0)):
        assert run(k_=kk, d_=dd) == INVALID
    for kk, dd in ((17, 256), (33, 1), (32, 129), (1, 257)):
        assert run(k_=kk, d_=dd, ld=kk + 2 * kk * dd) == UNSUPPORTED, (kk, dd)
    assert run(n_=0) == INVALID and run(n_=2 ** 31) == UNSUPPORTED
    assert run(ld=14) == INVALID and b"k + 2 k d" in lib.d3p_last_error()
    assert run(rows_=2 ** 32) == UNSUPPORTED and b"2^32" in lib.d3p_last_error()
    assert run(out_=C.c_void_p(out.data_ptr() + 4)) == INVALID and b"aligned to 8" in lib.d3p_last_error()
    host = np.zeros(64)
    hp = C.c_void_p(host.ctypes.data)
    assert run(x_=hp) == INVALID and run(lat_=hp) == INVALID and run(out_=hp) == INVALID and b"device memory" in lib.d3p_last_error()
    assert run(ws_=None) == INVALID and b"workspace" in lib.d3p_last_error()
    assert run(ws_=C.c_void_p(ws.data_ptr() + 4)) == INVALID and b"workspace" in lib.d3p_last_error()
    assert run(ws_=hp) == INVALID and b"workspace" in lib.d3p_last_error()
    assert run(bytes_=nbytes - 1) == INVALID and b"workspace" in lib.d3p_last_error()
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((ws == CANARY).all())              # nothing was launched
    assert run() == 0
    torch.cuda.synchronize()
    got = np_(out[1:1 + n])
    # x = 0, mus = sigs = 1, equal weights: ll = -d (1 / 2 + log(2 pi) / 2) in every row, in float32: a handful of roundings at a
    # magnitude below 4 (ulp 2^-22), 16 2^-23 allowed per row
    assert np.all(got == got[0]) and abs(got[0] + rows * d * (0.5 + G.HALF_LOG_2PI)) <= rows * 16 * 2.0 ** -23
    assert float(out[0]) == CANARY and float(out[-1]) == CANARY and float(ws[0]) == CANARY and float(ws[-1]) == CANARY


# ---------------------------------------------------------------- log_likelihood_total and log_joint
def _toy(k=3, d=2, rows=257, seed=4):
    """obs around k modes, and guide parameters near them."""
    r = np.random.default_rng([seed, k, d, rows])
    modes = (4.0 * r.normal(size=(k, d))).astype(np.float32)
    z = r.integers(0, k, rows)
    obs = (modes[z] + 0.7 * r.normal(size=(rows, d))).astype(np.float32)
    params = {"alpha_log": (np.log(30.0) + 0.3 * r.normal(size=k)).astype(np.float32), "mus_loc": modes}
    return obs, params


@pytest.mark.parametrize("k,d,rows,n", [(3, 2, 257, 65), (16, 5, 70, 7)])
def test_totals_and_log_joint_against_the_reference(MDG, k, d, rows, n):
    from d3p_amd import mixture as MX
    from d3p_amd import mixture_density as MD
    tau = 7.5
    m, g = _mg(prior_mu_scale=tau)
    obs, params = _toy(k, d, rows)
    x = torch.tensor(obs).cuda()
    tp = {name: torch.tensor(v) for name, v in params.items()}
    draws = MX.posterior_predictive_samples(P.key(21), n, m, (k, x), g, tp)
    s = {name: draws[name] for name in ("pis", "mus", "sigs")}
    assert MD._packed_view(s["pis"], s["mus"], s["sigs"], n, k, d, x.device) is not None       # views of one buffer: read in place
    ll = np_(MD.log_likelihood(m, s, x)["obs"])
    tot, lj = MDG.log_likelihood_total(m, s, x), MDG.log_joint(m, s, x)
    for t in (tot, lj):
        assert t.shape == (n,) and t.dtype == torch.float64 and t.is_cuda
    assert_sums(np_(tot), ll, f"k={k} d={d} log_likelihood_total")
    pis, mus, sigs = (np_(s[name]) for name in ("pis", "mus", "sigs"))
    want = R.log_joint(G.totals(ll), k, mus, sigs, tau)
    bound = G.totals_bound(ll) + R.density_bound(k, d, pis, mus, sigs, params["alpha_log"], params["mus_loc"], tau, True) + 4 * G.U53 * np.abs(want)
    err = np.abs(np_(lj) - want)
    print(f"k={k} d={d} log_joint: largest error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # unpacked samples (numpy, sigs broadcast over the draws' last axis kept whole): the copying path gives the same bits
    unpacked = {"pis": pis.copy(), "mus": mus.copy(), "sigs": sigs.copy()}
    assert torch.equal(MDG.log_likelihood_total(m, unpacked, obs), tot) and torch.equal(MDG.log_joint(m, unpacked, obs), lj)
    empty = MDG.log_likelihood_total(m, unpacked, np.zeros((0, d), np.float32))
    assert empty.shape == (n,) and bool((empty == 0.0).all())


# ---------------------------------------------------------------- guide_diagnostic
def _check_totals(res, n, what):
    """elbo, elbo_se, log_evidence_is and ess against the reference on the device's own pointwise ratios; the float64 rounding bounds
    of tests/test_gpu_guide_diag.py: a sum of n terms errs by n 2^-53 sum |terms|; the variance by (n + 4) 2^-52 of itself plus the
    effect of the rounded mean; the log-sum-exp and the ess are sums of n exponentials: (n + 8) 2^-52 relative."""
    lr = np_(res.pointwise["log_ratio"])
    st = G.stats(lr)
    tol = (n + 8) * 2.0 ** -52
    for t in (res.elbo, res.elbo_se, res.log_evidence_is, res.pareto_k, res.ess):
        assert t.dtype == torch.float64 and t.dim() == 0 and t.is_cuda
    assert abs(float(res.elbo) - st["elbo"]) <= n * G.U53 * np.abs(lr).sum() / n + G.U53 * abs(st["elbo"]), what
    if n == 1:
        assert math.isnan(float(res.elbo_se)) and math.isnan(st["elbo_se"])
    else:
        mean_err = G.U53 * np.abs(lr).sum()
        var_slack = 2.0 * mean_err * np.abs(lr - st["elbo"]).sum() / (n - 1) / n
        assert abs(float(res.elbo_se) ** 2 - st["elbo_se"] ** 2) <= tol * st["elbo_se"] ** 2 + var_slack, what
    assert abs(float(res.log_evidence_is) - st["log_evidence_is"]) <= tol + 2.0 * G.U53 * abs(st["log_evidence_is"]), what
    assert abs(float(res.ess) - st["ess"]) <= 4.0 * tol * st["ess"], what
    assert float(res.log_evidence_is) >= float(res.elbo) - tol * abs(float(res.elbo))
    assert set(res.pointwise) == {"log_ratio", "log_joint", "log_q", "log_likelihood"}
    for name in res.pointwise:
        assert res.pointwise[name].shape == (n,) and res.pointwise[name].dtype == torch.float64 and res.pointwise[name].is_cuda


def _check_k(res, what):
    lr = np_(res.pointwise["log_ratio"])
    k, cond = G.pareto_k(lr, with_cond=True)
    got = float(res.pareto_k)
    if not np.isfinite(k):
        assert got == k or (math.isnan(got) and math.isnan(k)), f"{what}: pareto_k {got!r} against {k!r}"
        return
    bound = PR.bounds(np.array([0.0]), np.array([0.0]), np.array([k]), np.array([cond]))[2][0]
    print(f"{what}: pareto_k {got:.6f} against {k:.6f}, error / bound {abs(got - k) / bound:.3f}")
    assert abs(got - k) <= bound, f"{what}: pareto_k {got!r} against {k!r} (bound {bound:.3e})"


def test_guide_diagnostic_uses_the_draws_of_the_predictive(MDG):
    from d3p_amd import mixture as MX
    from d3p_amd.criteria import _k_threshold
    k, d, rows, n, tau = 3, 2, 257, 128, 10.0
    m, g = _mg()
    obs, params = _toy(k, d, rows)
    x = torch.tensor(obs).cuda()
    tp = {name: torch.tensor(v) for name, v in params.items()}
    key = P.key(77)
    res = MDG.guide_diagnostic(key, n, m, (k, x, rows), g, tp, pointwise=True)
    assert res.n_draws == n and res.n_rows == rows and res.k_threshold == _k_threshold(n)
    draws = MX.posterior_predictive_samples(key, n, m, (k, x), g, tp)
    s = {name: draws[name] for name in ("pis", "mus", "sigs")}
    assert torch.equal(res.pointwise["log_likelihood"], MDG.log_likelihood_total(m, s, x))          # bit for bit: the same latents
    assert torch.equal(res.pointwise["log_joint"], MDG.log_joint(m, s, x))
    pis, mus, sigs = (np_(s[name]) for name in ("pis", "mus", "sigs"))
    tot = np_(res.pointwise["log_likelihood"])
    want = R.log_ratio(tot, k, pis, mus, params["alpha_log"], params["mus_loc"], tau)
    bound = R.density_bound(k, d, pis, mus, sigs, params["alpha_log"], params["mus_loc"], tau, False) + 6 * G.U53 * (np.abs(tot) + np.abs(want))
    err = np.abs(np_(res.pointwise["log_ratio"]) - want)
    print(f"log_ratio: largest error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # log_q carries the sigs terms, log_ratio does not: equal up to their rounding, not bitwise
    diff = np_(res.pointwise["log_joint"] - res.pointwise["log_q"]) - np_(res.pointwise["log_ratio"])
    assert np.all(np.abs(diff) <= 8 * G.U53 * (np.abs(np_(res.pointwise["log_joint"])) + np.abs(np_(res.pointwise["log_q"]))))
    _check_totals(res, n, "toy")
    _check_k(res, "toy")
    short = MDG.guide_diagnostic(key, n, m, (k, x), g, tp)
    assert short.pointwise is None and all(np_(a).tobytes() == np_(b).tobytes() for a, b in zip((short[0], short[1], short[2], short[3], short[5]),
                                                                                                (res[0], res[1], res[2], res[3], res[5])))
    kw = MDG.guide_diagnostic(key, n, m, (k,), g, tp, obs=x, num_obs_total=rows)
    assert np_(kw.elbo).tobytes() == np_(res.elbo).tobytes()
    other = MDG.guide_diagnostic(P.key(78), n, m, (k, x), g, tp, pointwise=True)
    assert not torch.equal(other.pointwise["log_ratio"], res.pointwise["log_ratio"])


@pytest.mark.parametrize("n", [1, 20, 21, 128, 1000])
def test_guide_diagnostic_at_every_draw_count(MDG, n):
    """n = 1: the standard error is NaN; n <= 20: no tail of five draws, pareto_k = +inf; n = 21: the first fit."""
    m, g = _mg()
    obs, params = _toy()
    res = MDG.guide_diagnostic(P.key(5), n, m, (3, torch.tensor(obs).cuda()), g, {k_: torch.tensor(v) for k_, v in params.items()}, pointwise=True)
    _check_totals(res, n, f"n={n}")
    _check_k(res, f"n={n}")
    assert math.isnan(float(res.elbo_se)) == (n == 1)
    assert (float(res.pareto_k) == math.inf) == (n <= 20) and (n <= 20 or math.isfinite(float(res.pareto_k)))


def test_special_ratios(MDG, monkeypatch):
    """Patched draws: one draw repeated (every ratio equal: pareto_k = -inf); a NaN (every total NaN); and pis_j == 0 in one draw at
    alpha_j < 1 (a -inf ratio: elbo = -inf, pareto_k = +inf, log_evidence_is finite), alpha_j == 1 (nothing) and alpha_j > 1 (a +inf
    ratio: elbo = log_evidence_is = +inf, pareto_k = +inf, elbo_se and ess NaN)."""
    from d3p_amd import mixture_density as MD
    m, g = _mg()
    obs, params = _toy()
    x = torch.tensor(obs).cuda()
    real = MD._posterior_latents
    state = {}

    def planted(*a, **kw):
        out = real(*a, **kw)
        state["fill"](out[3])
        return out
    monkeypatch.setattr(MD, "_posterior_latents", planted)

    def run(n, alpha0=None, pointwise=True):
        p = {k_: torch.tensor(v) for k_, v in params.items()}
        if alpha0 is not None:
            p["alpha_log"] = p["alpha_log"].clone()
            p["alpha_log"][0] = math.log(alpha0)
        return MDG.guide_diagnostic(P.key(9), n, m, (3, x), g, p, pointwise=pointwise)

    state["fill"] = lambda latent: latent.copy_(latent[:1].expand_as(latent).clone())
    for n in (2, 64):
        res = run(n)
        lr = np_(res.pointwise["log_ratio"])
        assert np.all(lr == lr[0]) and np.isfinite(lr[0])
        assert float(res.pareto_k) == -math.inf and float(res.elbo) == lr[0] and float(res.elbo_se) == 0.0 and float(res.ess) == n
    assert float(run(1).pareto_k) == math.inf                              # one draw: nothing to compare

    def zero_weight(latent):                                               # draw 5: the first weight 0, the others renormalised
        latent[5, 0] = 0.0
        latent[5, 1:3] /= latent[5, 1:3].sum()
    state["fill"] = zero_weight
    res = run(30, alpha0=0.5)
    lr = np_(res.pointwise["log_ratio"])
    assert np.isneginf(lr).sum() == 1 and lr[5] == -np.inf and np_(res.pointwise["log_q"])[5] == np.inf
    assert np.isfinite(np_(res.pointwise["log_likelihood"])).all()         # the likelihood only drops the component
    assert float(res.elbo) == -math.inf and float(res.pareto_k) == math.inf and math.isfinite(float(res.log_evidence_is))
    assert abs(float(res.log_evidence_is) - G.stats(lr)["log_evidence_is"]) <= 40 * 2.0 ** -52 * abs(float(res.log_evidence_is))
    res = run(30, alpha0=1.0)
    assert np.isfinite(np_(res.pointwise["log_ratio"])).all() and all(math.isfinite(float(v)) for v in (res.elbo, res.elbo_se, res.log_evidence_is,
                                                                                                     res.pareto_k, res.ess))
    _check_totals(res, 30, "alpha_j == 1 with a zero weight")
    _check_k(res, "alpha_j == 1 with a zero weight")
    res = run(30, alpha0=2.0)
    lr = np_(res.pointwise["log_ratio"])
    assert np.isposinf(lr).sum() == 1 and lr[5] == np.inf
    assert float(res.elbo) == math.inf and float(res.log_evidence_is) == math.inf and float(res.pareto_k) == math.inf
    assert math.isnan(float(res.elbo_se)) and math.isnan(float(res.ess))
    state["fill"] = lambda latent: latent.__setitem__((7, 4), math.nan)    # a NaN in a mean of draw 7
    res = run(30, pointwise=False)
    assert all(math.isnan(float(v)) for v in (res.elbo, res.elbo_se, res.log_evidence_is, res.pareto_k, res.ess))


def test_moving_the_guide_off_the_modes_lowers_the_elbo(MDG):
    """The guide's scales are fixed, so it cannot be widened; moving mus_loc a few units away from the fitted modes must lower the
    ELBO.  The order only, on the same key (the same standard normals and scales in both runs)."""
    m, g = _mg()
    obs, params = _toy(3, 2, 600)
    x = torch.tensor(obs).cuda()
    fitted = {k_: torch.tensor(v) for k_, v in params.items()}
    moved = dict(fitted, mus_loc=fitted["mus_loc"] + 3.0)
    a = MDG.guide_diagnostic(P.key(13), 64, m, (3, x), g, fitted)
    b = MDG.guide_diagnostic(P.key(13), 64, m, (3, x), g, moved)
    print(f"elbo at the modes {float(a.elbo):.1f}, moved by 3 units {float(b.elbo):.1f}")
    assert math.isfinite(float(a.elbo)) and math.isfinite(float(b.elbo)) and float(b.elbo) < float(a.elbo)


# ---------------------------------------------------------------- example
def test_example_prints_the_diagnostic_line(MDG, capsys):
    spec = importlib.util.spec_from_file_location("ex_gmm_diag", os.path.join(ROOT, "examples", "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args([]).guide_diagnostic is None and mod.parse_args(["--guide-diagnostic"]).guide_diagnostic == 100
    mod.main(mod.parse_args("--sigma 1.0 -N 512 -n 2 --guide-diagnostic 64".split()))
    out = capsys.readouterr().out
    num = r"(-?[\d.]+|-?inf|nan)"
    hit = re.search(r"guide diagnostic \(512 rows, 64 draws\): elbo " + num + r" \+- " + num + r", log_evidence_is " + num +
                    r", pareto k " + num + r" \(threshold " + num + r"\), ess " + num, out)
    assert hit, out
    elbo, se, lis, k, thr, ess = (float(v) for v in hit.groups())
    assert math.isfinite(elbo) and se >= 0.0 and lis >= elbo - 0.01 and 1.0 <= ess <= 64.0 and not math.isnan(k)
    assert "assignment accuracy: " in out
