"""d3p_amd.diagnostics on the GPU: d3p_loglik_draw_sums against the float64 row sums of THE DEVICE'S OWN rows-form matrix (that
matrix is pinned by tests/loglik_ref.py, so only the new reduction is judged) within the float64 reordering bound
rows 2^-53 sum_r |ll[s, r]| -- derived, not measured; its determinism, special values, extents and refusals; log_joint and
log_likelihood_total against tests/guide_diag_ref.py; guide_diagnostic's draws, totals and Pareto k; and the two examples' flag."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import guide_diag_ref as G
from tests import loglik_ref as LR
from tests import predictive_ref as P
from tests import psis_ref as PR
from tests import waic_ref as WR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 12345.0
ROWS = (1, 63, 64, 65, 127, 128, 129, 257)
NS = (1, 31, 32, 33, 64, 65, 128, 129, 257)
DS = (1, 4, 31, 32, 33, 65)


def np_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def DG(gpu):
    from d3p_amd import diagnostics
    return diagnostics


def make_model(family, d, intercept, **kw):
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    if family == "logistic":
        return LogisticRegression(d, intercept=intercept, **kw)
    if family == "linear":
        kw.setdefault("obs_scale", LR.SIGMA["linear"])
        return LinearRegression(d, intercept=intercept, **kw)
    return PoissonRegression(d, intercept=intercept, **kw)


def samples_of(W, b):
    s = {"w": torch.tensor(np.array(W)).cuda()}
    if b is not None:
        s["intercept"] = torch.tensor(np.array(b)).cuda()
    return s


def rows_matrix(model, s, Xt, yt):
    """The device's own (n, rows) float32 matrix, as numpy."""
    from d3p_amd import infer_util as U
    return np_(next(iter(U.log_likelihood(model, s, Xt, yt).values())))


def strips_of(rows):
    tiles = -(-rows // 128)
    per = -(-tiles // 512) if tiles else 0
    return (-(-tiles // per), per) if tiles else (0, 0)


def draw_sums_entry(model, X, y, W, b, pad=16):
    """d3p_loglik_draw_sums on numpy inputs with the latents at a padded leading dimension (intercept in column 0, weights from
    column 2, canaries elsewhere) and canaries on both sides of the output and of the workspace: (n,) float64 numpy after the
    canaries were checked."""
    import d3p_amd._lib as L
    from d3p_amd import infer_util as U
    lib = L.load()
    rows, d = X.shape
    n = W.shape[0]
    ld = d + 5
    lat = torch.full((n, ld), CANARY, device="cuda")
    lat[:, 2:2 + d] = torch.tensor(W).cuda()
    if b is not None:
        lat[:, 0] = torch.tensor(b).cuda()
    before = lat.clone()
    nbytes = lib.d3p_loglik_draw_sums_workspace(rows, n)
    assert nbytes == 8 * strips_of(rows)[0] * n
    out = torch.full((n + 2 * pad,), CANARY, dtype=torch.float64, device="cuda")
    ws = torch.full((nbytes // 8 + 2 * pad,), CANARY, dtype=torch.float64, device="cuda")
    ms = U._model_struct(model, U._family(model), d)
    Xt, yt = torch.tensor(X).cuda(), torch.tensor(y).cuda()
    L.check(lib.d3p_loglik_draw_sums(L.stream_ptr(), C.byref(ms), L.ptr(Xt), L.ptr(yt), rows, L.ptr(lat), ld, 2, 0 if b is not None else -1, n,
                                     L.ptr(out[pad:]), L.ptr(ws[pad:]), nbytes))
    torch.cuda.synchronize()
    assert bool((out[:pad] == CANARY).all()) and bool((out[pad + n:] == CANARY).all()), "the output was written outside its extent"
    assert bool((ws[:pad] == CANARY).all()) and bool((ws[pad + nbytes // 8:] == CANARY).all()), "the workspace was written outside its extent"
    assert torch.equal(lat, before)
    return np_(out[pad:pad + n]).copy()


def assert_sums(got, ll, what):
    """got (n,) float64 against the float64 row sums of ll (n, rows) float32 within rows 2^-53 sum |ll|; draws whose sum is not
    finite agree exactly."""
    ref, bound = G.totals(ll), G.totals_bound(ll)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), what + ": the non-finite draws differ"
    err = np.abs(got[fin] - ref[fin])
    if fin.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"{what}: largest error / bound {np.nanmax(np.where(bound[fin] > 0, err / bound[fin], 0.0)):.3f}, "
                  f"largest relative error {np.max(err / np.maximum(np.abs(ref[fin]), 1e-300)):.2e}")
    assert np.all(err <= bound[fin]), f"{what}: error {err.max():.3e} above the bound"


def sweep_cases():
    """(family, n, rows, d, intercept): nine cases per family; every value of ROWS, NS and DS occurs for every family (nine
    consecutive indices cover each axis), both intercept settings for every family."""
    out = []
    for f, family in enumerate(LR.FAMILIES):
        for i in range(9):
            out.append((family, NS[(i + 2 * f) % 9], ROWS[(i + f) % 8], DS[(i + 3 * f) % 6], bool((i + f) % 2)))
    return out


def test_the_sweep_covers_every_axis_value_for_every_family():
    for family in LR.FAMILIES:
        mine = [c for c in sweep_cases() if c[0] == family]
        assert {c[1] for c in mine} == set(NS) and {c[2] for c in mine} == set(ROWS) and {c[3] for c in mine} == set(DS)
        assert {c[4] for c in mine} == {False, True}


# ---------------------------------------------------------------- the entry against its comparator
def _direct_case(family, n, rows, d, intercept, seed=None):
    X, y, W, b = LR.inputs(family, n, rows, d, intercept, seed=seed)
    model = make_model(family, d, intercept)
    ll = rows_matrix(model, samples_of(W, b), torch.tensor(X).cuda(), torch.tensor(y).cuda())
    return model, X, y, W, b, ll


@pytest.mark.parametrize("family,n,rows,d,intercept", sweep_cases())
def test_draw_sums_at_tile_edges(gpu, family, n, rows, d, intercept):
    model, X, y, W, b, ll = _direct_case(family, n, rows, d, intercept)
    assert ll.shape == (n, rows) and np.isfinite(ll).all()
    got = draw_sums_entry(model, X, y, W, b)
    assert_sums(got, ll, f"{family} n={n} rows={rows} d={d} intercept={intercept}")


@pytest.mark.parametrize("family,n,rows,d,intercept,what", [
    ("linear", 3, 1025 * 128 - 5, 4, True, "three row tiles per workgroup"),        # tiles = 1025: per = 3, 342 strips, the last of 2 tiles
    ("poisson", 130, 300, 33, True, "three strips, a ragged last tile"),            # tiles = 3 = strips, the last of 44 rows; two draw tiles
    ("logistic", 33, 512 * 128 - 37, 4, False, "the largest strip count"),          # tiles = 512 = strips, the last ragged
])
def test_draw_sums_over_strips(gpu, family, n, rows, d, intercept, what):
    strips, per = strips_of(rows)
    assert {"three row tiles per workgroup": per == 3 and strips == 342, "three strips, a ragged last tile": strips == 3 and rows % 128,
            "the largest strip count": strips == 512 and per == 1 and rows % 128}[what]
    model, X, y, W, b, ll = _direct_case(family, n, rows, d, intercept, seed=61)
    got = draw_sums_entry(model, X, y, W, b)
    assert_sums(got, ll, what)
    again = draw_sums_entry(model, X, y, W, b)
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), "two calls differ"


def test_draw_sums_do_not_depend_on_the_other_draws(gpu):
    """The same table with draws appended: the first n sums keep their bits (130 draws against their first 70 and first 1)."""
    model, X, y, W, b, _ = _direct_case("poisson", 130, 300, 33, True, seed=61)
    whole = draw_sums_entry(model, X, y, W, b)
    for n in (70, 1):
        part = draw_sums_entry(model, X, y, np.ascontiguousarray(W[:n]), np.ascontiguousarray(b[:n]))
        assert np.array_equal(whole[:n].view(np.int64), part.view(np.int64)), n


# ---------------------------------------------------------------- special values
def test_a_poisson_rate_that_overflows_makes_that_draw_minus_infinity(gpu):
    n, rows, d, X, y, W, t = WR.overflow_problem(False)
    assert (t[2] > 89.0).sum() == 9 and not (np.delete(t, 2, axis=0) > 80.0).any()
    model = make_model("poisson", d, False)
    ll = rows_matrix(model, samples_of(W, None), torch.tensor(X).cuda(), torch.tensor(y).cuda())
    assert np.isneginf(ll[2]).sum() == 9 and np.isfinite(np.delete(ll, 2, axis=0)).all()
    got = draw_sums_entry(model, X, y, W, None)
    assert got[2] == -np.inf and np.isfinite(np.delete(got, 2)).all()
    assert_sums(got, ll, "one draw overflows")


@pytest.mark.parametrize("family", LR.FAMILIES)
def test_a_nan_in_x_makes_every_draw_nan(gpu, family):
    X, y, W, b = LR.inputs(family, 70, 131, 5, True, seed=23)
    X = X.copy()
    X[70, 3] = np.nan
    got = draw_sums_entry(make_model(family, 5, True), X, y, W, b)
    assert np.isnan(got).all()


def test_no_rows_give_zeros_without_a_launch(gpu):
    import d3p_amd._lib as L
    from d3p_amd import infer_util as U
    lib = L.load()
    model = make_model("poisson", 3, False)
    ms = U._model_struct(model, U._family(model), 3)
    X, y, lat = torch.zeros((1, 3), device="cuda"), torch.zeros(1, device="cuda"), torch.zeros((5, 3), device="cuda")
    out = torch.full((9,), CANARY, dtype=torch.float64, device="cuda")
    assert lib.d3p_loglik_draw_sums_workspace(0, 5) == 0
    assert lib.d3p_loglik_draw_sums(L.stream_ptr(), C.byref(ms), L.ptr(X), L.ptr(y), 0, L.ptr(lat), 3, 0, -1, 5, L.ptr(out[2:]), None, 0) == 0
    torch.cuda.synchronize()
    assert bool((out[2:7] == 0.0).all()) and bool((out[:2] == CANARY).all()) and bool((out[7:] == CANARY).all())


# ---------------------------------------------------------------- refusals
def test_c_entry_refuses_before_any_launch(gpu):
    import d3p_amd._lib as L
    from d3p_amd import infer_util as U
    lib = L.load()
    rows, d, n = 40, 3, 6
    X, y = torch.zeros((rows, d), device="cuda"), torch.zeros(rows, device="cuda")
    lat = torch.zeros((n, d + 1), device="cuda")
    out = torch.full((n + 2,), CANARY, dtype=torch.float64, device="cuda")
    nbytes = lib.d3p_loglik_draw_sums_workspace(rows, n)
    assert nbytes == 8 * n
    ws = torch.full((n + 2,), CANARY, dtype=torch.float64, device="cuda")
    plain = make_model("logistic", d, False)
    ms = U._model_struct(plain, U._family(plain), d)

    def run(ms_=ms, X_=L.ptr(X), y_=L.ptr(y), rows_=rows, lat_=L.ptr(lat), ld=d + 1, w_off=0, b_col=-1, n_=n, out_=L.ptr(out[1:]),
            ws_=L.ptr(ws[1:]), bytes_=nbytes):
        return lib.d3p_loglik_draw_sums(L.stream_ptr(), C.byref(ms_), X_, y_, rows_, lat_, ld, w_off, b_col, n_, out_, ws_, bytes_)
    assert run(bytes_=nbytes - 1) == -1 and b"workspace" in lib.d3p_last_error()
    assert run(ws_=None) == -1 and b"workspace" in lib.d3p_last_error()
    assert run(ws_=C.c_void_p(ws.data_ptr() + 4)) == -1 and b"workspace" in lib.d3p_last_error()
    host = np.zeros(n + 2)
    assert run(ws_=C.c_void_p(host.ctypes.data)) == -1 and b"workspace" in lib.d3p_last_error()
    assert run(out_=C.c_void_p(out.data_ptr() + 4)) == -1 and b"aligned to 8" in lib.d3p_last_error()
    assert run(out_=None) == -1 and run(X_=None) == -1 and run(lat_=None) == -1 and run(n_=0) == -1
    assert run(b_col=d) == -1 and b"intercept" in lib.d3p_last_error()              # b_col without an intercept
    with_b = make_model("logistic", d, True)
    assert run(ms_=U._model_struct(with_b, U._family(with_b), d)) == -1 and b"intercept" in lib.d3p_last_error()   # and the reverse
    assert run(w_off=2) == -1
    gauss = L.LogregModel(d, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_GAUSS_MEAN, L.D3P_GUIDE_SOFTPLUS, 1.0)
    assert run(ms_=gauss) == -3
    sites = L.LogregModel(d, 1, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LOGREG, L.D3P_GUIDE_EXP_SITES, 0.0)
    assert run(ms_=sites, b_col=d) == -3
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((ws == CANARY).all())              # nothing was launched
    assert run() == 0
    torch.cuda.synchronize()
    got = np_(out[1:1 + n])                                                           # every t = 0: ll = float32(-log 2) in every row
    assert np.all(got == got[0]) and abs(got[0] + rows * math.log(2.0)) <= rows * 2.0 ** -23
    assert float(out[0]) == CANARY and float(out[-1]) == CANARY and float(ws[0]) == CANARY and float(ws[-1]) == CANARY


# ---------------------------------------------------------------- log_likelihood_total and log_joint
@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("family", LR.FAMILIES)
def test_totals_and_log_joint_against_the_reference(DG, family, intercept):
    n, rows, d = 65, 257, 33
    X, y, W, b = LR.inputs(family, n, rows, d, intercept)
    model = make_model(family, d, intercept, prior_scale=1.7, intercept_prior_scale=0.6)
    Xt, yt, s = torch.tensor(X).cuda(), torch.tensor(y).cuda(), samples_of(W, b)
    ll = rows_matrix(model, s, Xt, yt)
    tot = DG.log_likelihood_total(model, s, Xt, yt, rows)
    lj = DG.log_joint(model, s, Xt, yt)
    for t in (tot, lj):
        assert t.shape == (n,) and t.dtype == torch.float64 and t.is_cuda
    assert_sums(np_(tot), ll, f"{family} intercept={intercept} log_likelihood_total")
    want = G.totals(ll) + G.log_prior(W, b, 1.7, 0.6)
    bound = G.totals_bound(ll) + G.prior_bound(W, b, 1.7, 0.6) + G.U53 * np.abs(want)     # (+ the rounding of the last addition)
    err = np.abs(np_(lj) - want)
    print(f"{family} intercept={intercept} log_joint: largest error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    assert torch.equal(DG.log_likelihood_total(model, {k: np_(v) for k, v in s.items()}, X, y), tot)      # numpy inputs: the copying path
    # a single sample: 0-d
    one = {"w": s["w"][3]}
    if intercept:
        one["intercept"] = s["intercept"][3]
    t1, j1 = DG.log_likelihood_total(model, one, Xt, yt), DG.log_joint(model, one, Xt, yt)
    assert t1.dim() == 0 and j1.dim() == 0 and t1.dtype == torch.float64
    assert float(t1) == float(tot[3]) and abs(float(j1) - want[3]) <= bound[3]


# ---------------------------------------------------------------- guide_diagnostic
def _guide_case(family, kind, d=4, rows=257, seed=12, scale=0.2):
    from d3p_amd.models import AutoDiagonalNormal, DiagonalNormalGuide, MeanFieldGuide
    model = make_model(family, d, True)
    guide = {"auto": AutoDiagonalNormal, "meanfield": MeanFieldGuide}[kind](model) if kind != "diagonal" else DiagonalNormalGuide(model, site="w")
    raw = P.logreg_params(guide, d, True, np.random.default_rng(seed))
    raw = {k: (np.float32(scale) * v if k.endswith("_loc") else v) for k, v in raw.items()}     # (keeps the Poisson rates moderate)
    params = {k: torch.tensor(v) for k, v in raw.items()}
    X, y, _, _ = LR.inputs(family, 1, rows, d, True, seed=41)
    return model, guide, params, raw, torch.tensor(X).cuda(), torch.tensor(y).cuda()


def _latents(key, n, model, guide, params, Xt):
    from d3p_amd import modelling as M
    from d3p_amd import predictive as PS
    from d3p_amd.models import LogisticRegression
    if isinstance(model, LogisticRegression):
        return M.sample_multi_posterior_predictive(key, n, model, (Xt,), guide, (Xt,), params)
    return PS.posterior_predictive_samples(key, n, model, (Xt,), guide, params)


def _check_totals(res, n, what):
    """elbo, elbo_se, log_evidence_is and ess against the reference on the device's own pointwise ratios.  Bounds, float64 rounding:
    a sum of n terms errs by n 2^-53 sum |terms|; the variance by (n + 4) 2^-52 of itself (deviations from a rounded mean, squares, their
    sum, two divisions), its root by half that; the log-sum-exp and the ess are sums of n exponentials of exactly representable
    differences (one ulp each, then n additions): (n + 8) 2^-52 relative for the sums, so that much absolute for the logarithm."""
    lr = np_(res.pointwise["log_ratio"])
    st = G.stats(lr)
    tol = (n + 8) * 2.0 ** -52
    for t in (res.elbo, res.elbo_se, res.log_evidence_is, res.pareto_k, res.ess):
        assert t.dtype == torch.float64 and t.dim() == 0 and t.is_cuda
    assert abs(float(res.elbo) - st["elbo"]) <= n * G.U53 * np.abs(lr).sum() / n + G.U53 * abs(st["elbo"]), what
    if n == 1:
        assert math.isnan(float(res.elbo_se)) and math.isnan(st["elbo_se"])
    else:
        mean_err = G.U53 * np.abs(lr).sum()                            # of the rounded mean: it moves every deviation
        dev = np.abs(lr - st["elbo"])
        var_slack = 2.0 * mean_err * dev.sum() / (n - 1) / n
        assert abs(float(res.elbo_se) ** 2 - st["elbo_se"] ** 2) <= tol * st["elbo_se"] ** 2 + var_slack, what
    assert abs(float(res.log_evidence_is) - st["log_evidence_is"]) <= tol + 2.0 * G.U53 * abs(st["log_evidence_is"]), what
    assert abs(float(res.ess) - st["ess"]) <= 4.0 * tol * st["ess"], what
    assert float(res.log_evidence_is) >= float(res.elbo) - tol * abs(float(res.elbo))
    pw = res.pointwise
    assert torch.equal(pw["log_ratio"], pw["log_joint"] - pw["log_q"])
    for name in ("log_ratio", "log_joint", "log_q", "log_likelihood"):
        assert pw[name].shape == (n,) and pw[name].dtype == torch.float64 and pw[name].is_cuda


def _check_k(res, what):
    lr = np_(res.pointwise["log_ratio"])
    k, cond = G.pareto_k(lr, with_cond=True)
    got = float(res.pareto_k)
    if not np.isfinite(k):
        assert got == k or (math.isnan(got) and math.isnan(k)), f"{what}: pareto_k {got!r} against {k!r}"
        return
    # d3p_psis_loo rounds k to float32; the float64 result is that float32 value
    bound = PR.bounds(np.array([0.0]), np.array([0.0]), np.array([k]), np.array([cond]))[2][0]
    print(f"{what}: pareto_k {got:.6f} against {k:.6f}, error / bound {abs(got - k) / bound:.3f}")
    assert abs(got - k) <= bound, f"{what}: pareto_k {got!r} against {k!r} (bound {bound:.3e})"


@pytest.mark.parametrize("family,kind", [("logistic", "auto"), ("logistic", "diagonal"), ("logistic", "meanfield"), ("linear", "auto"),
                                         ("linear", "diagonal"), ("poisson", "auto"), ("poisson", "diagonal")])
def test_guide_diagnostic_uses_the_draws_of_the_predictive(DG, family, kind):
    from d3p_amd.criteria import _k_threshold
    model, guide, params, raw, Xt, yt = _guide_case(family, kind)
    n, rows, d, key = 128, 257, 4, P.key(77)
    res = DG.guide_diagnostic(key, n, model, (Xt, yt, rows), guide, params, pointwise=True)
    assert res.n_draws == n and res.n_rows == rows and res.k_threshold == _k_threshold(n)
    draws = _latents(key, n, model, guide, params, Xt)
    s = {"w": draws["w"], "intercept": draws["intercept"]}
    assert torch.equal(res.pointwise["log_likelihood"], DG.log_likelihood_total(model, s, Xt, yt))          # bit for bit
    assert torch.equal(res.pointwise["log_joint"], DG.log_joint(model, s, Xt, yt))
    W, b = np_(s["w"]).reshape(n, d), np_(s["intercept"]).reshape(n)
    loc, sigma = G.guide_loc_sigma(kind, raw, d, True)
    lq = G.log_q(np.concatenate([W, b[:, None]], axis=1), loc, sigma)
    terms = 0.5 * ((np.concatenate([W, b[:, None]], axis=1) - loc) / sigma) ** 2
    q_bound = 2.0 * (d + 5) * G.U53 * (terms.sum(axis=1) + np.abs(np.log(sigma)).sum() + (d + 1) * G.HALF_LOG_2PI) + \
        2.0 ** -52 * (terms * 2.0).sum(axis=1)                          # (as prior_bound; + one ulp of (theta - loc) / sigma, squared)
    assert np.all(np.abs(np_(res.pointwise["log_q"]) - lq) <= q_bound), f"log_q: {np.max(np.abs(np_(res.pointwise['log_q']) - lq) / q_bound)}"
    _check_totals(res, n, f"{family} {kind}")
    _check_k(res, f"{family} {kind}")
    assert np.isfinite(float(res.pareto_k))
    short = DG.guide_diagnostic(key, n, model, (Xt, yt), guide, params)
    assert short.pointwise is None and all(np_(a).tobytes() == np_(b_).tobytes() for a, b_ in zip((short[0], short[1], short[2], short[3], short[5]),
                                                                                                 (res[0], res[1], res[2], res[3], res[5])))
    other = DG.guide_diagnostic(P.key(78), n, model, (Xt, yt), guide, params, pointwise=True)
    assert not torch.equal(other.pointwise["log_ratio"], res.pointwise["log_ratio"])


@pytest.mark.parametrize("n", [1, 20, 21, 128, 1000])
def test_guide_diagnostic_at_every_draw_count(DG, n):
    """n = 1: the standard error is NaN; n <= 20: no tail of five draws, pareto_k = +inf; n = 21: the first fit."""
    model, guide, params, raw, Xt, yt = _guide_case("poisson", "auto")
    res = DG.guide_diagnostic(P.key(5), n, model, (Xt, yt), guide, params, pointwise=True)
    _check_totals(res, n, f"n={n}")
    _check_k(res, f"n={n}")
    assert math.isnan(float(res.elbo_se)) == (n == 1)
    assert (float(res.pareto_k) == math.inf) == (n <= 20) and (n <= 20 or math.isfinite(float(res.pareto_k)))


def test_equal_ratios_report_minus_infinity(DG, monkeypatch):
    """One draw repeated: every ratio is exactly equal -- the guide 'is' the posterior as far as these draws can tell."""
    from d3p_amd import infer_util as U
    model, guide, params, raw, Xt, yt = _guide_case("linear", "auto")
    real = U._guide_latents

    def repeated(key, n, *a, **k):
        latent, ld, w_off, b_col = real(key, n, *a, **k)
        latent.copy_(latent[:1].expand_as(latent).clone())
        return latent, ld, w_off, b_col
    monkeypatch.setattr(U, "_guide_latents", repeated)
    for n in (2, 64):
        res = DG.guide_diagnostic(P.key(9), n, model, (Xt, yt), guide, params, pointwise=True)
        lr = np_(res.pointwise["log_ratio"])
        assert np.all(lr == lr[0]) and np.isfinite(lr[0])
        assert float(res.pareto_k) == -math.inf and float(res.elbo) == lr[0] and float(res.elbo_se) == 0.0
        assert float(res.log_evidence_is) == pytest.approx(lr[0], abs=2.0 ** -50 * abs(lr[0])) and float(res.ess) == n
        _check_k(res, "equal ratios")
    res = DG.guide_diagnostic(P.key(9), 1, model, (Xt, yt), guide, params)
    assert float(res.pareto_k) == math.inf                              # one draw: nothing to compare


def test_special_ratios(DG, monkeypatch):
    """A -inf ratio (a Poisson rate that overflows in one draw): elbo = -inf, pareto_k = +inf, log_evidence_is finite; every ratio
    -inf: log_evidence_is = -inf too; a NaN: every total NaN."""
    from d3p_amd import infer_util as U
    n_, rows, d, X, y, W, t = WR.overflow_problem(False)
    from d3p_amd.models import AutoDiagonalNormal
    model = make_model("poisson", d, False)
    guide = AutoDiagonalNormal(model)
    params = {"auto_loc": torch.zeros(d), "auto_scale": torch.ones(d)}
    Xt, yt = torch.tensor(X).cuda(), torch.tensor(y).cuda()
    real = U._guide_latents
    state = {}

    def planted(key, n, *a, **k):
        latent, ld, w_off, b_col = real(key, n, *a, **k)
        state["fill"](latent)
        return latent, ld, w_off, b_col
    monkeypatch.setattr(U, "_guide_latents", planted)
    Wt = torch.tensor(W).cuda()

    def some(latent):
        latent[:5, :d] = Wt
        latent[5:, :d] = Wt[0]
    state["fill"] = some
    res = DG.guide_diagnostic(P.key(1), 30, model, (Xt, yt), guide, params, pointwise=True)
    lr = np_(res.pointwise["log_ratio"])
    assert np.isneginf(lr).sum() == 1 and lr[2] == -np.inf
    assert float(res.elbo) == -math.inf and float(res.pareto_k) == math.inf and math.isfinite(float(res.log_evidence_is))
    assert abs(float(res.log_evidence_is) - G.stats(lr)["log_evidence_is"]) <= 40 * 2.0 ** -52 * abs(float(res.log_evidence_is))
    state["fill"] = lambda latent: latent.__setitem__((slice(None), slice(0, d)), Wt[2])
    res = DG.guide_diagnostic(P.key(1), 30, model, (Xt, yt), guide, params)
    assert float(res.elbo) == -math.inf and float(res.pareto_k) == math.inf and float(res.log_evidence_is) == -math.inf
    state["fill"] = lambda latent: (some(latent), latent.__setitem__((7, 1), math.nan))
    res = DG.guide_diagnostic(P.key(1), 30, model, (Xt, yt), guide, params)
    assert all(math.isnan(float(v)) for v in (res.elbo, res.elbo_se, res.log_evidence_is, res.pareto_k, res.ess))


@pytest.mark.parametrize("c2", [0.5, 1.5])
def test_orthogonal_linear_case_lands_where_the_theory_puts_it(DG, c2):
    """The host test's closed form on the device: D = 1, 64 rows, the guide Normal(m, c / sqrt(P)) in float32, 4096 draws.  log r_s -
    log p(y | X) follows D log c + (1 - c^2) / 2 z^2 up to the float32 likelihood, and pareto_k lies on the side of the threshold the
    host test established column by column: below it for both, above 0 for the narrow guide, below 0 for the wide one."""
    from d3p_amd.models import AutoDiagonalNormal, LinearRegression
    prob = G.orthogonal_problem(1, 64)
    model = LinearRegression(1, prior_scale=G.ORTHO_TAU, intercept=False, obs_scale=G.ORTHO_SIGMA)
    loc, sigma = G.scaled_posterior_guide(prob, math.sqrt(c2))
    params = {"auto_loc": torch.tensor(loc.astype(np.float32)), "auto_scale": torch.tensor(sigma.astype(np.float32))}
    Xt, yt = torch.tensor(prob["X"]).cuda(), torch.tensor(prob["y"]).cuda()
    n = 4096
    res = DG.guide_diagnostic(P.key(3), n, model, (Xt, yt), AutoDiagonalNormal(model), params, pointwise=True)
    _check_totals(res, n, f"orthogonal c^2={c2}")
    _check_k(res, f"orthogonal c^2={c2}")
    k = float(res.pareto_k)
    assert k < res.k_threshold == 0.7 and ((0.0 < k) if c2 < 1.0 else (k < 0.0))
    # the elbo sits below the evidence by the closed form's mean, -(D log c + (1 - c^2) / 2): within 5 standard errors and the float32 slack
    gap = prob["log_evidence"] + math.log(math.sqrt(c2)) + 0.5 * (1.0 - c2) - float(res.elbo)
    assert abs(gap) <= 5.0 * float(res.elbo_se) + 1e-3


# ---------------------------------------------------------------- examples
@pytest.mark.parametrize("name", ["linear_regression", "poisson_regression"])
def test_examples_print_the_diagnostic_line(gpu, name):
    cmd = [sys.executable, os.path.join(ROOT, "examples", name + ".py"), "--num-steps", "50", "-N", "2000", "--guide-diagnostic", "64"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    num = r"(-?[\d.]+|-?inf|nan)"
    m = re.search(r"guide diagnostic \(2000 rows, 64 draws\): elbo " + num + r" \+- " + num + r", log_evidence_is " + num +
                  r", pareto k " + num + r" \(threshold " + num + r"\), ess " + num, out.stdout)
    assert m, out.stdout
    elbo, se, lis, k, thr, ess = (float(v) for v in m.groups())
    assert math.isfinite(elbo) and se >= 0.0 and lis >= elbo - 0.01 and 1.0 <= ess <= 64.0 and not math.isnan(k)
    assert "loss per example" in out.stdout
