"""d3p_amd.criteria on the GPU against tests/waic_ref.py (float64 numpy; the bound of p_waic is derived and calibrated there):
pointwise p_waic and elpd_waic within their bounds at every tile edge of both kernels, lppd bit-identical to the log predictive
density of the sibling modules, the totals against numpy float64 of the device's own pointwise arrays, exact zeros for equal draws,
the special values (Poisson overflow, NaN), the posterior forms against the explicit path bit for bit, compare, and the C entries'
refusals and output extents."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import loglik_ref as LR
from tests import mixture_density_ref as MR
from tests import mixture_ref as R
from tests import predictive_ref as P
from tests import waic_ref as WR

pytestmark = pytest.mark.gpu
T, DT = MR.T, MR.DT
POINTWISE = ("lppd", "p_waic", "elpd_waic")


def np_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def CR(gpu):
    from d3p_amd import criteria
    return criteria


def make_model(family, d, intercept):
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    if family == "logistic":
        return LogisticRegression(d, intercept=intercept)
    if family == "linear":
        return LinearRegression(d, intercept=intercept, obs_scale=LR.SIGMA["linear"])
    return PoissonRegression(d, intercept=intercept)


def samples_of(W, b):
    s = {"w": torch.tensor(np.array(W)).cuda()}
    if b is not None:
        s["intercept"] = torch.tensor(np.array(b)).cuda()
    return s


def _mg():
    from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel
    m = GaussianMixtureModel()
    return m, GaussianMixtureGuide(m)


def _mix_samples(ref):
    return {name: np.array(ref[name]) for name in ("pis", "mus", "sigs")}   # (copies: the shared reference is read-only)


def _same_bits(a, b):
    for name in POINTWISE:
        assert np.array_equal(np_(a.pointwise[name]).view(np.int32), np_(b.pointwise[name]).view(np.int32)), name
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(np_(x).view(np.int64), np_(y).view(np.int64))
    assert a[4:6] == b[4:6]


def _check_result(res, ref, n, rows, lppd_dev, what):
    assert res.n_draws == n and res.n_rows == rows and sorted(res.pointwise) == sorted(POINTWISE)
    for name in POINTWISE:
        assert res.pointwise[name].shape == (rows,) and res.pointwise[name].dtype == torch.float32 and res.pointwise[name].is_cuda
    assert torch.equal(res.pointwise["lppd"], lppd_dev), what + ": lppd differs from log_predictive_density"
    WR.assert_within(np_(res.pointwise["p_waic"]), ref["v"], ref["bound_v"], what + " p_waic")
    WR.assert_within(np_(res.pointwise["elpd_waic"]), ref["elpd"], ref["elpd_bound"], what + " elpd_waic")
    WR.check_totals(res, what)


# ---------------------------------------------------------------- regression families: tile-edge sweep
@pytest.mark.parametrize("family,n,rows,d,intercept", LR.sweep_cases())
def test_regression_at_tile_edges(CR, family, n, rows, d, intercept):
    """n in {1, 31, 128, 129, 257}, rows in {1, 63, 128, 129, 300}, d in {1, 31, 32, 33, 513}: the draw tile, the row tile, the K
    slice and the half-wave from below, exactly and from above; n <= 64 leaves the wm = 1 wave without a draw (the count-0 branch
    of the merge).  ddof = 1; the n = 1 cases run at ddof = 0, where p_waic is exactly 0."""
    from d3p_amd import infer_util as U
    ddof = 1 if n >= 2 else 0
    ref = WR.regression_reference(family, n, rows, d, intercept, ddof)
    model = make_model(family, d, intercept)
    Xt, yt, s = torch.tensor(np.array(ref["X"])).cuda(), torch.tensor(np.array(ref["y"])).cuda(), samples_of(ref["W"], ref.get("b"))
    what = f"{family} n={n} rows={rows} d={d} intercept={intercept} ddof={ddof}"
    res = CR.waic(model, s, Xt, yt, rows, ddof=ddof, pointwise=True)
    _check_result(res, ref, n, rows, U.log_predictive_density(model, s, Xt, yt, rows), what)
    if n == 1:
        assert bool((res.pointwise["p_waic"] == 0.0).all()) and torch.equal(res.pointwise["elpd_waic"], res.pointwise["lppd"])
    _same_bits(res, CR.waic(model, s, Xt, yt, rows, ddof=ddof, pointwise=True))
    short = CR.waic(model, s, Xt, yt, ddof=ddof)
    assert short.pointwise is None and float(short.elpd_waic) == float(res.elpd_waic) and float(short.p_waic) == float(res.p_waic)


# ---------------------------------------------------------------- mixture model: shapes, row edges, draw edges
@pytest.mark.parametrize("kind", MR.KINDS)
@pytest.mark.parametrize("k,d,rows,n", WR.MIXTURE_CASES)
def test_mixture_at_every_shape_and_edge(CR, k, d, rows, n, kind):
    """MR.CASES with n >= 2: every shape, the row tile's edges 63 / 64 / 65 / 129, the draw split 3 / 5 / 9 over four waves and 3 over
    two waves at the two largest shapes (a wave without a draw is skipped in the merge)."""
    from d3p_amd import mixture_density as MD
    ref = WR.mixture_reference(kind, k, d, rows, n, 1)
    m, _ = _mg()
    obs, s = np.array(ref["obs"]), _mix_samples(ref)
    what = f"{kind} k={k} d={d} rows={rows} n={n}"
    res = CR.waic(m, s, obs, ddof=1, pointwise=True)
    _check_result(res, ref, n, rows, MD.log_predictive_density(m, s, obs), what)
    _same_bits(res, CR.waic(m, s, obs, ddof=1, pointwise=True))
    pop = CR.waic(m, s, obs, ddof=0, pointwise=True)
    ref0 = WR.mixture_reference(kind, k, d, rows, n, 0)
    WR.assert_within(np_(pop.pointwise["p_waic"]), ref0["v"], ref0["bound_v"], what + " p_waic at ddof = 0")
    assert torch.equal(pop.pointwise["lppd"], res.pointwise["lppd"])


# ---------------------------------------------------------------- equal draws
@pytest.mark.parametrize("family", LR.FAMILIES)
def test_equal_draws_give_exactly_zero_regression(CR, family):
    """n = 130 identical draws: both wm waves and two draw tiles take part, every shifted sum is 0 and so is the merge."""
    n, rows, d = 130, 150, 33
    X, y, W, b = LR.inputs(family, 1, rows, d, True, seed=17)
    s = samples_of(np.repeat(W, n, axis=0), np.repeat(b, n))
    for ddof in (0, 1):
        res = CR.waic(make_model(family, d, True), s, torch.tensor(X).cuda(), torch.tensor(y).cuda(), ddof=ddof, pointwise=True)
        pw = np_(res.pointwise["p_waic"])
        assert np.all(pw == 0.0) and not np.signbit(pw).any(), family
        assert torch.equal(res.pointwise["elpd_waic"], res.pointwise["lppd"]) and float(res.p_waic) == 0.0


def test_equal_draws_give_exactly_zero_mixture(CR):
    n, k, d, rows = 130, 3, 5, T + 1
    obs, pis, mus, sigs = MR.soft_inputs(k, d, rows, 1)
    m, _ = _mg()
    s = {"pis": np.repeat(pis, n, axis=0), "mus": np.repeat(mus, n, axis=0), "sigs": np.repeat(sigs, n, axis=0)}
    for ddof in (0, 1):
        res = CR.waic(m, s, obs, ddof=ddof, pointwise=True)
        assert bool((res.pointwise["p_waic"] == 0.0).all()) and torch.equal(res.pointwise["elpd_waic"], res.pointwise["lppd"])


# ---------------------------------------------------------------- Poisson overflow
def _overflow_reference(all_draws):
    n, rows, d, X, y, W, t = WR.overflow_problem(all_draws)
    ll = LR.ll64("poisson", X, y, W, None, 1.0)
    bound = LR.ll_bound("poisson", X, y, W, None, 1.0, ll)
    lppd = LR.lppd64(ll)
    v = WR.pwaic64(ll, 1)
    bv = WR.bound_v(ll, bound.max(axis=0), 1, v)
    lb = LR.lppd_bound(ll, bound, lppd)
    return n, rows, d, X, y, W, t, ll, lppd, lb, v, bv


def test_poisson_overflow_in_one_draw(CR):
    from d3p_amd import infer_util as U
    n, rows, d, X, y, W, t, ll, lppd, lb, v, bv = _overflow_reference(False)
    hit = t[2] > 89.0
    assert hit.sum() == 9 and np.array_equal(np.isneginf(ll).any(axis=0), hit) and np.isfinite(lppd).all()
    model = make_model("poisson", d, False)
    Xt, yt, s = torch.tensor(X).cuda(), torch.tensor(y).cuda(), samples_of(W, None)
    res = CR.waic(model, s, Xt, yt, pointwise=True)
    got = {name: np_(res.pointwise[name]) for name in POINTWISE}
    assert not any(np.isnan(a).any() for a in got.values())
    assert np.isfinite(got["lppd"]).all() and torch.equal(res.pointwise["lppd"], U.log_predictive_density(model, s, Xt, yt))
    assert np.all(got["p_waic"][hit] == np.inf) and np.all(got["elpd_waic"][hit] == -np.inf)
    LR.assert_close(got["lppd"], lppd, lb, "one draw overflows, lppd")
    WR.assert_within(got["p_waic"], v, bv, "one draw overflows, p_waic")            # (the hit rows by equality, the others within bounds)
    WR.assert_within(got["elpd_waic"], lppd - v, lb + bv, "one draw overflows, elpd_waic")
    assert float(res.elpd_waic) == -np.inf and float(res.p_waic) == np.inf and float(res.waic) == np.inf


def test_poisson_overflow_in_every_draw(CR):
    n, rows, d, X, y, W, t, ll, lppd, lb, v, bv = _overflow_reference(True)
    dead = (t > 89.0).all(axis=0)
    assert dead.sum() == 10 and np.array_equal(np.isneginf(lppd), dead)
    res = CR.waic(make_model("poisson", d, False), samples_of(W, None), torch.tensor(X).cuda(), torch.tensor(y).cuda(), pointwise=True)
    got = {name: np_(res.pointwise[name]) for name in POINTWISE}
    assert not any(np.isnan(a).any() for a in got.values())
    assert np.all(got["lppd"][dead] == -np.inf) and np.all(got["p_waic"][dead] == np.inf) and np.all(got["elpd_waic"][dead] == -np.inf)
    LR.assert_close(got["lppd"], lppd, lb, "every draw overflows, lppd")
    WR.assert_within(got["p_waic"], v, bv, "every draw overflows, p_waic")
    WR.assert_within(got["elpd_waic"], lppd - v, lb + bv, "every draw overflows, elpd_waic")


# ---------------------------------------------------------------- NaN
@pytest.mark.parametrize("family", LR.FAMILIES)
def test_a_nan_in_x_makes_exactly_that_row_nan(CR, family):
    n, rows, d = 129, 131, 5
    X, y, W, b = LR.inputs(family, n, rows, d, True, seed=23)
    model, s, yt = make_model(family, d, True), samples_of(W, b), torch.tensor(y).cuda()
    base = CR.waic(model, s, torch.tensor(X).cuda(), yt, pointwise=True)
    X = X.copy()
    X[70, 3] = np.nan
    res = CR.waic(model, s, torch.tensor(X).cuda(), yt, pointwise=True)
    keep = np.arange(rows) != 70
    for name in POINTWISE:
        got = np_(res.pointwise[name])
        assert np.isnan(got[70]) and np.array_equal(got[keep], np_(base.pointwise[name])[keep]), name
    assert all(np.isnan(float(t)) for t in res[:4])


def test_a_nan_in_obs_makes_exactly_that_row_nan_mixture(CR):
    obs, pis, mus, sigs = (np.array(v) for v in MR.soft_inputs(3, 2, T + 3, 6))
    m, _ = _mg()
    s = {"pis": pis, "mus": mus, "sigs": sigs}
    base = CR.waic(m, s, obs, pointwise=True)
    obs[T + 1, 1] = np.nan
    res = CR.waic(m, s, obs, pointwise=True)
    keep = np.arange(T + 3) != T + 1
    for name in POINTWISE:
        got = np_(res.pointwise[name])
        assert np.isnan(got[T + 1]) and np.array_equal(got[keep], np_(base.pointwise[name])[keep]), name
    # a draw whose every component is -inf: the rows' p_waic is +inf, lppd stays finite
    p1 = pis.copy()
    p1[2] = 0.0
    dead = CR.waic(m, {"pis": p1, "mus": mus, "sigs": sigs}, MR.soft_inputs(3, 2, T + 3, 6)[0], pointwise=True)
    assert bool(torch.isfinite(dead.pointwise["lppd"]).all()) and bool((dead.pointwise["p_waic"] == np.inf).all())
    assert bool((dead.pointwise["elpd_waic"] == -np.inf).all())


# ---------------------------------------------------------------- posterior forms
@pytest.mark.parametrize("family", LR.FAMILIES)
def test_posterior_waic_draws_the_latents_of_the_predictive(CR, family):
    """Same key, same n: the latents are sample_multi_posterior_predictive's (predictive.posterior_predictive_samples returns them
    for the three families), the kernel is the same -- bit for bit."""
    from d3p_amd import predictive as PS
    from d3p_amd.models import AutoDiagonalNormal
    n, rows, d = 5, 70, 4
    X, y, _, _ = LR.inputs(family, 1, rows, d, True, seed=41)
    model = make_model(family, d, True)
    guide = AutoDiagonalNormal(model)
    params = {k: torch.tensor(v) for k, v in P.logreg_params(guide, d, True, np.random.default_rng(12)).items()}
    params["auto_loc"] = 0.2 * params["auto_loc"]                 # (keeps the Poisson rates moderate)
    Xt, yt, key = torch.tensor(X).cuda(), torch.tensor(y).cuda(), P.key(77)
    draws = PS.posterior_predictive_samples(key, n, model, (Xt,), guide, params)
    want = CR.waic(model, {"w": draws["w"], "intercept": draws["intercept"]}, Xt, yt, pointwise=True)
    got = CR.posterior_waic(key, n, model, (Xt, yt, rows), guide, params, pointwise=True)
    assert got.n_draws == n and got.n_rows == rows and bool(torch.isfinite(got.pointwise["elpd_waic"]).all())
    _same_bits(got, want)
    other = CR.posterior_waic(P.key(78), n, model, (Xt, yt), guide, params, ddof=0, pointwise=True)
    assert not torch.equal(other.pointwise["p_waic"], got.pointwise["p_waic"])


def test_posterior_waic_mixture_draws_the_latents_of_the_predictive(CR):
    from d3p_amd import mixture as MX
    m, g = _mg()
    k, d, rows, n = 3, 2, T + 5, 6
    obs = MR.soft_inputs(k, d, rows, 1)[0]
    params, args, key = R.posterior_params(k, d, 5), (k, obs, rows, d), R.key(31)
    samples = MX.posterior_predictive_samples(key, n, m, args, g, params)
    want = CR.waic(m, {name: samples[name] for name in ("pis", "mus", "sigs")}, obs, pointwise=True)
    got = CR.posterior_waic(key, n, m, args, g, params, pointwise=True)
    assert got.n_draws == n and got.n_rows == rows
    _same_bits(got, want)
    kw = CR.posterior_waic(key, n, m, (k, None), g, params, pointwise=True, obs=obs)
    _same_bits(kw, want)


# ---------------------------------------------------------------- compare
def test_compare_poisson_against_linear_on_the_same_draws(CR):
    """Nothing is fitted: the Poisson and the linear likelihood of the same counts under the same draws, against numpy float64 of
    the pointwise arrays."""
    from d3p_amd.models import LinearRegression, PoissonRegression
    n, rows, d = 31, 129, 33
    X, y, W, b = LR.inputs("poisson", n, rows, d, True)
    Xt, yt, s = torch.tensor(X).cuda(), torch.tensor(y).cuda(), samples_of(W, b)
    a = CR.waic(PoissonRegression(d, intercept=True), s, Xt, yt, pointwise=True)
    lin = CR.waic(LinearRegression(d, intercept=True, obs_scale=LR.SIGMA["linear"]), s, Xt, yt, pointwise=True)
    got = CR.compare(a, lin)
    assert got.elpd_diff.is_cuda and got.elpd_diff.dtype == torch.float64 and got.se_diff.dim() == 0
    diff = np_(a.pointwise["elpd_waic"]).astype(np.float64) - np_(lin.pointwise["elpd_waic"]).astype(np.float64)
    terms = rows * (diff - diff.mean()) ** 2 / (rows - 1)
    print(f"elpd_diff {float(got.elpd_diff):.4f} +- {float(got.se_diff):.4f} (numpy: {diff.sum():.4f}, {np.sqrt(terms.sum()):.4f})")
    assert abs(float(got.elpd_diff) - diff.sum()) <= WR.sum_bound(diff)
    assert abs(float(got.se_diff) ** 2 - terms.sum()) <= WR.sum_bound(terms) + 2.0 ** -51 * terms.sum()
    assert float(got.se_diff) > 0.0 and float(CR.compare(lin, a).elpd_diff) == -float(got.elpd_diff)
    with pytest.raises(ValueError):
        CR.compare(a, CR.waic(PoissonRegression(d, intercept=True), s, Xt, yt))


# ---------------------------------------------------------------- C entries
CANARY = 12345.0


def test_c_entries_refuse_as_declared_and_stay_inside_their_buffers(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    n, rows, d, pad = 129, 130, 5, 512
    X, y, W, b = LR.inputs("linear", n, rows, d, True, seed=8)
    Xt, yt = torch.tensor(X).cuda(), torch.tensor(y).cuda()
    lat = torch.tensor(np.concatenate([W, b[:, None]], axis=1)).cuda()
    ms = L.LogregModel(d, 1, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LINREG, 0, LR.SIGMA["linear"])
    buf = torch.full((2 * rows + 3 * pad,), CANARY, device="cuda")
    lp, pw = buf[pad:pad + rows], buf[2 * pad + rows:2 * pad + 2 * rows]

    def reg(n_=n, ddof=1, rows_=rows, lp_=lp, pw_=pw, ms_=ms):
        b_col = d if ms_.intercept else -1
        return lib.d3p_loglik_waic(L.stream_ptr(), C.byref(ms_), L.ptr(Xt), L.ptr(yt), rows_, L.ptr(lat), d + 1, 0, b_col, n_, ddof, L.ptr(lp_), L.ptr(pw_))
    assert reg(ddof=2) == -1 and b"ddof" in lib.d3p_last_error()
    assert reg(n_=1, ddof=1) == -1 and reg(n_=0, ddof=0) == -1 and reg(pw_=None) == -1 and reg(lp_=None) == -1
    assert reg(ms_=L.LogregModel(d, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_GAUSS_MEAN, 0, 1.0)) == -3
    assert reg(ms_=L.LogregModel(d, 1, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LOGREG, L.D3P_GUIDE_EXP_SITES, 0.0)) == -3
    assert reg(rows_=0) == 0
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())                                                   # nothing was launched
    assert reg() == 0
    torch.cuda.synchronize()
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[pad:pad + rows] = True
    inside[2 * pad + rows:2 * pad + 2 * rows] = True
    assert bool((buf[~inside] == CANARY).all()) and not bool((buf[inside] == CANARY).any())

    k, dd, mrows, mn = 3, 2, T + 1, DT + 1
    obs, pis, mus, sigs = MR.soft_inputs(k, dd, mrows, mn)
    x = torch.tensor(obs).cuda()
    ld = k + 2 * k * dd + 3
    mlat = torch.zeros((mn, ld), device="cuda")
    mlat[:, :k], mlat[:, k:k + k * dd], mlat[:, k + k * dd:k + 2 * k * dd] = (torch.tensor(pis).cuda(), torch.tensor(mus).cuda().reshape(mn, -1),
                                                                              torch.tensor(sigs).cuda().reshape(mn, -1))
    mbuf = torch.full((2 * mrows + 3 * pad,), CANARY, device="cuda")
    mlp, mpw = mbuf[pad:pad + mrows], mbuf[2 * pad + mrows:2 * pad + 2 * mrows]

    def mix(n_=mn, ddof=1, rows_=mrows, lp_=mlp, pw_=mpw, k_=k, ld_=ld):
        return lib.d3p_gmm_loglik_waic(L.stream_ptr(), L.ptr(x), rows_, dd, L.ptr(mlat), ld_, k_, n_, ddof, L.ptr(lp_), L.ptr(pw_))
    assert mix(ddof=2) == -1 and b"ddof" in lib.d3p_last_error()
    assert mix(n_=1, ddof=1) == -1 and mix(n_=0, ddof=0) == -1 and mix(pw_=None) == -1 and mix(lp_=None) == -1 and mix(ld_=14) == -1
    assert mix(k_=33) == -3 and mix(n_=2 ** 31) == -3
    assert mix(rows_=0) == 0
    torch.cuda.synchronize()
    assert bool((mbuf == CANARY).all())
    assert mix() == 0
    torch.cuda.synchronize()
    inside = torch.zeros_like(mbuf, dtype=torch.bool)
    inside[pad:pad + mrows] = True
    inside[2 * pad + mrows:2 * pad + 2 * mrows] = True
    assert bool((mbuf[~inside] == CANARY).all()) and not bool((mbuf[inside] == CANARY).any())


# ---------------------------------------------------------------- examples
def _example(name):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ex_waic_" + name, os.path.join(root, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_poisson_example_reports_waic_behind_its_flag(CR, capsys):
    import argparse
    import re
    mod = _example("poisson_regression")
    args = argparse.Namespace(sigma=0.5, clip_threshold=1.0, num_steps=300, learning_rate=2e-2, batch_size=200, dimensions=4, num_samples=2000)
    plain = mod.main(args)
    off = capsys.readouterr().out
    assert "WAIC" not in off and "elpd" not in off                             # off by default: the output is what it was
    args.waic, args.posterior_draws = True, 7
    assert mod.main(args) == plain
    out = capsys.readouterr().out
    assert out.startswith(off)
    num = r"(-?[\d.]+)"
    lines = [re.search(name + r" WAIC \(2000 rows, 7 posterior draws\): elpd_waic " + num + r" \+- " + num + r", p_waic " + num, out)
             for name in ("Poisson", "linear")]
    diff = re.search(r"Poisson against linear on the same counts: elpd_diff " + num + r" \+- " + num, out)
    assert all(lines) and diff
    values = [float(v) for m in lines for v in m.groups()] + [float(v) for v in diff.groups()]
    assert np.isfinite(values).all() and abs(values[6] - (values[0] - values[3])) <= 0.02   # (two decimals are printed)


def test_mixture_example_reports_waic_behind_its_flag(CR, capsys):
    import re
    mod = _example("gaussian_mixture_model")
    assert mod.parse_args([]).waic is False                                    # off by default
    args = mod.parse_args("--sigma 1.0 -N 512 -n 2 --waic --posterior-draws 7".split())
    mod.main(args)
    out = capsys.readouterr().out
    m = re.search(r"WAIC \(512 points, 7 posterior draws\): elpd_waic (-?[\d.]+) \+- ([\d.]+), p_waic ([\d.]+)", out)
    assert m and np.isfinite([float(v) for v in m.groups()]).all() and "held-out" not in out
