"""PSIS-LOO on the GPU (d3p_psis_loo, d3p_amd.criteria.loo / posterior_loo) against tests/psis_ref.py applied to THE DEVICE'S OWN
float32 log-likelihood matrix -- that matrix is pinned by tests/loglik_ref.py and tests/mixture_density_ref.py, so only the new
arithmetic is judged.  Bound per value: 2^-24 |v| + the float64 term calibrated in psis_ref (its docstring); rows whose reference is
not finite (k = +inf: no fit; -inf; NaN) must agree exactly.  The tail itself is not an output of the entry, so its membership
is not compared directly: it is judged through the k = +inf rows (T <= 4 against T >= 5) and through k, which depends on T, e_1 and
e_q and so moves by far more than its bound when a draw changes sides of the cut.  elpd does NOT pin membership on the near-tied
matrices (every x there lies within 1e-6 of 0, so elpd barely moves); the exactness of the selection on such columns rests on k and
on psis_ref's kernel-order restatement, whose membership is asserted equal to the reference's on the CPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import loglik_ref as LR
from tests import mixture_density_ref as MR
from tests import mixture_ref as R
from tests import predictive_ref as P
from tests import psis_ref as PR

pytestmark = pytest.mark.gpu
POINTWISE = ("elpd_loo", "p_loo", "lppd", "pareto_k")
CANARY = 12345.0


def np_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def CR(gpu):
    from d3p_amd import criteria
    return criteria


def psis_entry(ll, ld=None, pad=64):
    """d3p_psis_loo on the (n, rows) numpy matrix ll at leading dimension ld, canaries in the matrix's padding and around the three
    outputs: (elpd, lppd, k) numpy float32 after the canaries were checked."""
    import d3p_amd._lib as L
    n, rows = ll.shape
    ld = rows if ld is None else ld
    mat = torch.full((n, ld), CANARY, device="cuda")
    mat[:, :rows] = torch.tensor(ll).cuda()
    out = torch.full((3 * rows + 4 * pad,), CANARY, device="cuda")
    views = [out[pad + i * (rows + pad):pad + i * (rows + pad) + rows] for i in range(3)]
    L.check(L.load().d3p_psis_loo(L.stream_ptr(), L.ptr(mat), ld, n, rows, *(L.ptr(v) for v in views)))
    torch.cuda.synchronize()
    inside = torch.zeros_like(out, dtype=torch.bool)
    for i in range(3):
        inside[pad + i * (rows + pad):pad + i * (rows + pad) + rows] = True
    assert bool((out[~inside] == CANARY).all()), "an output was written outside its extent"
    assert bool((mat[:, rows:] == CANARY).all()) and np.array_equal(np_(mat[:, :rows]).view(np.int32), ll.view(np.int32))
    return tuple(np_(v).copy() for v in views)


def assert_matches(got, ll, what):
    """(elpd, lppd, k) of the device against psis_ref on the same float32 matrix."""
    elpd, lppd, k, T, cond = PR.psis_matrix(ll)
    be, bl, bk = PR.bounds(elpd, lppd, k, cond)
    for name, g, ref, b in (("elpd", got[0], elpd, be), ("lppd", got[1], lppd, bl), ("k", got[2], k, bk)):
        ok = PR.within(g, ref, b)
        fin = np.isfinite(ref)
        if fin.any():
            with np.errstate(invalid="ignore"):
                ratio = np.abs(g.astype(np.float64) - ref)[fin] / b[fin]
                ulps = np.abs(g.astype(np.float64) - ref)[fin] / (PR.ROUND32 * np.maximum(np.abs(ref[fin]), 1e-300))
            print(f"{what} {name}: largest error / bound {ratio.max():.3f}, largest error / (2^-24 |v|) {ulps.max():.3f}")
        bad = np.nonzero(~ok)[0]
        assert bad.size == 0, f"{what} {name}: row {bad[0]}: {g[bad[0]]!r} against {ref[bad[0]]!r} (bound {b[bad[0]]:.3e}, T = {T[bad[0]]})"
    assert np.array_equal(np.isposinf(got[2]), np.isposinf(k)), what + ": the rows without a fit differ"


# ---------------------------------------------------------------- the entry alone, model-free
@pytest.mark.parametrize("n,rows", PR.direct_cases())
def test_direct_entry_on_random_and_near_tied_matrices(gpu, n, rows):
    """Every n at which M or the branch changes (1, 2, 5 | 6, 20 | 21: the first fit; 25 | 26; the draw lanes' 8 and the strided
    partials' 64 from below, exactly and from above; 225 | 226: n / 5 against 3 sqrt n; 1000; 4097) with every row count around the
    workgroup's 32 rows (1, 63, 64, 65, 127, 128, 129, 257), ll_ld > rows.  Not the full cross product: psis_ref.direct_cases pairs every
    n with two of the row counts (34 cases; every n and every row count occurs, each row count with at least four n) -- the kernel's
    handling of the draws (per column) and of the rows (the workgroup's 32) do not interact, and each case stays within seconds."""
    for kind, make in (("random", PR.random_matrix), ("near_tied", PR.near_tied_matrix)):
        ll = make(n, rows, 1)
        got = psis_entry(ll, ld=rows + 5)
        assert_matches(got, ll, f"{kind} n={n} rows={rows}")
        again = psis_entry(ll, ld=rows + 5)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, again)), "two calls differ"
        if rows > 40:                                                  # a row's result does not depend on the launch's other rows
            part = psis_entry(np.ascontiguousarray(ll[:, 33:40]))
            assert all(np.array_equal(a[33:40].view(np.int32), b.view(np.int32)) for a, b in zip(got, part)), "rows 33..39 alone differ"


def test_direct_entry_at_the_largest_n_with_indices_past_2_to_31(gpu):
    """n = 65535 (M = 768, the whole of the kernel's LDS plan), 2 rows, at a leading dimension that puts the last draws' elements
    beyond 2^31 floats."""
    import d3p_amd._lib as L
    n, rows, ld = 65535, 2, 32800
    assert (n - 1) * ld > 2 ** 31 and PR.tail_len(n) == 768
    ll = PR.random_matrix(n, rows, 3)
    mat = torch.empty((n, ld), device="cuda")
    mat[:, :rows] = torch.tensor(ll).cuda()
    out = torch.full((3, rows + 2), CANARY, device="cuda")
    L.check(L.load().d3p_psis_loo(L.stream_ptr(), L.ptr(mat), ld, n, rows, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2])))
    torch.cuda.synchronize()
    assert bool((out[:, rows:] == CANARY).all())
    got = tuple(np_(out[i, :rows]) for i in range(3))
    assert np.isfinite(got[2]).all()
    assert_matches(got, ll, "n=65535")


def test_fixed_input_columns(gpu):
    ll = PR.fixed_columns()
    got = psis_entry(ll, ld=ll.shape[1] + 3)
    assert_matches(got, ll, "fixed columns")
    col = {name: tuple(float(g[c]) for g in got) for c, name in enumerate(PR.FIXED_NAMES)}
    assert col["equal"] == (-1.25, -1.25, np.inf)
    assert col["one_neg_inf"][0] == -np.inf and np.isfinite(col["one_neg_inf"][1]) and col["one_neg_inf"][2] == np.inf
    assert col["all_neg_inf"] == (-np.inf, -np.inf, np.inf)
    assert all(np.isnan(v) for v in col["one_nan"])
    assert np.isnan(col["one_pos_inf"][0]) and col["one_pos_inf"][1] == np.inf and np.isnan(col["one_pos_inf"][2])
    assert all(np.isfinite(v) for v in col["ties"] + col["low_cut"] + col["plain"])


def test_c_entry_refuses_as_declared(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    n, rows = 9, 40
    mat = torch.zeros((n, rows), device="cuda")
    out = torch.full((3, rows), CANARY, device="cuda")

    def run(mat_=L.ptr(mat), ld=rows, n_=n, rows_=rows, e=L.ptr(out[0]), lp=L.ptr(out[1]), k=L.ptr(out[2])):
        return lib.d3p_psis_loo(L.stream_ptr(), mat_, ld, n_, rows_, e, lp, k)
    odd = C.c_void_p(out[0].data_ptr() + 2)
    assert run(mat_=None) == -1 and run(e=None) == -1 and run(lp=None) == -1 and run(k=None) == -1
    assert run(e=odd) == -1 and b"aligned" in lib.d3p_last_error()
    assert run(n_=0) == -1 and run(n_=65536) == -1 and b"65535" in lib.d3p_last_error()
    assert run(ld=rows - 1) == -1 and b"ll_ld" in lib.d3p_last_error()
    assert run(rows_=0) == 0
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())                                 # nothing was launched
    assert run() == 0
    torch.cuda.synchronize()
    assert bool((out[0] == 0.0).all()) and bool((out[1] == 0.0).all()) and bool((out[2] == np.inf).all())


# ---------------------------------------------------------------- the families
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


def _same_bits(a, b):
    for name in POINTWISE:
        assert np.array_equal(np_(a.pointwise[name]).view(np.int32), np_(b.pointwise[name]).view(np.int32)), name
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(np_(x).view(np.int64), np_(y).view(np.int64))
    assert a[4:7] == b[4:7] and int(a.n_high_k) == int(b.n_high_k)


def _check_result(res, ll_dev, n, rows, waic_lppd, lppd_slack, what):
    """A LOOResult against psis_ref on the device's matrix, its totals against numpy float64 of its own pointwise arrays."""
    assert isinstance(res.k_threshold, float) and res.n_draws == n and res.n_rows == rows and sorted(res.pointwise) == sorted(POINTWISE)
    for name in POINTWISE:
        assert res.pointwise[name].shape == (rows,) and res.pointwise[name].dtype == torch.float32 and res.pointwise[name].is_cuda
    pw = {name: np_(res.pointwise[name]) for name in POINTWISE}
    assert_matches((pw["elpd_loo"], pw["lppd"], pw["pareto_k"]), np_(ll_dev), what)
    assert np.array_equal(pw["p_loo"], pw["lppd"] - pw["elpd_loo"])
    gap = np.abs(pw["lppd"].astype(np.float64) - np_(waic_lppd).astype(np.float64))
    assert np.all(gap <= lppd_slack), f"{what}: lppd is {gap.max():.3e} away from waic's"
    for t in res[:4]:
        assert t.dtype == torch.float64 and t.dim() == 0 and t.is_cuda
    e64, p64 = pw["elpd_loo"].astype(np.float64), pw["p_loo"].astype(np.float64)
    tol = rows * 2.0 ** -52
    assert abs(float(res.elpd_loo) - e64.sum()) <= tol * np.abs(e64).sum() and float(res.looic) == -2.0 * float(res.elpd_loo)
    assert abs(float(res.p_loo) - p64.sum()) <= tol * np.abs(p64).sum()
    terms = rows * (e64 - e64.mean()) ** 2 / (rows - 1)
    assert abs(float(res.se) ** 2 - terms.sum()) <= (tol + 2.0 ** -50) * terms.sum()
    assert res.k_threshold == min(1.0 - 1.0 / math.log10(n), 0.7)
    assert res.n_high_k.dtype == torch.int64 and res.n_high_k.dim() == 0 and res.n_high_k.is_cuda
    assert int(res.n_high_k) == int((~(pw["pareto_k"] <= res.k_threshold)).sum())


@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("d", [4, 33])
@pytest.mark.parametrize("family", LR.FAMILIES)
def test_regression_families(CR, family, d, intercept):
    from d3p_amd import infer_util as U
    n, rows = 64, 129
    X, y, W, b = LR.inputs(family, n, rows, d, intercept)
    model, Xt, yt, s = make_model(family, d, intercept), torch.tensor(X).cuda(), torch.tensor(y).cuda(), samples_of(W, b)
    ll = next(iter(U.log_likelihood(model, s, Xt, yt).values()))
    res = CR.loo(model, s, Xt, yt, rows, pointwise=True)
    w = CR.waic(model, s, Xt, yt, pointwise=True)
    slack = LR.LPPD_EXTRA * np.maximum(1.0, np.abs(np_(w.pointwise["lppd"]).astype(np.float64)))
    _check_result(res, ll, n, rows, w.pointwise["lppd"], slack, f"{family} d={d} intercept={intercept}")
    _same_bits(res, CR.loo(model, s, Xt, yt, pointwise=True))
    short = CR.loo(model, s, Xt, yt)
    assert short.pointwise is None and float(short.elpd_loo) == float(res.elpd_loo) and int(short.n_high_k) == int(res.n_high_k)


@pytest.mark.parametrize("k,d", [(3, 2), (16, 64)])
def test_mixture(CR, k, d):
    from d3p_amd import mixture_density as MD
    n, rows = 64, 129
    obs, pis, mus, sigs = (np.array(v) for v in MR.soft_inputs(k, d, rows, n))
    m, _ = _mg()
    s = {"pis": pis, "mus": mus, "sigs": sigs}
    ll = MD.log_likelihood(m, s, obs)["obs"]
    res = CR.loo(m, s, obs, pointwise=True)
    w = CR.waic(m, s, obs, pointwise=True)
    slack = 2.0 * MR.slack(np_(w.pointwise["lppd"]).astype(np.float64))   # (ll's slack and the reduction's)
    _check_result(res, ll, n, rows, w.pointwise["lppd"], slack, f"mixture k={k} d={d}")
    _same_bits(res, CR.loo(m, s, obs, pointwise=True))


# ---------------------------------------------------------------- slabs
def test_three_slabs_give_the_bits_of_one(CR):
    """rows = 300 at 128 rows per slab: 128, 128 and 44 rows -- through both dispatch paths."""
    n, rows, d = 64, 300, 33
    X, y, W, b = LR.inputs("poisson", n, rows, d, True, seed=51)
    model, Xt, yt, s = make_model("poisson", d, True), torch.tensor(X).cuda(), torch.tensor(y).cuda(), samples_of(W, b)
    whole = CR.loo(model, s, Xt, yt, pointwise=True)
    assert bool(torch.isfinite(whole.pointwise["elpd_loo"]).all())
    _same_bits(CR.loo(model, s, Xt, yt, pointwise=True, slab_bytes=4 * n * 128), whole)
    _same_bits(CR.loo(model, s, Xt, yt, pointwise=True, slab_bytes=1), whole)
    obs, pis, mus, sigs = (np.array(v) for v in MR.soft_inputs(3, 5, rows, n))
    m, _ = _mg()
    ms = {"pis": pis, "mus": mus, "sigs": sigs}
    whole = CR.loo(m, ms, obs, pointwise=True)
    _same_bits(CR.loo(m, ms, obs, pointwise=True, slab_bytes=4 * n * 128 + 100), whole)


# ---------------------------------------------------------------- posterior forms
@pytest.mark.parametrize("family", LR.FAMILIES)
def test_posterior_loo_draws_the_latents_of_the_predictive(CR, family):
    from d3p_amd import predictive as PS
    from d3p_amd.models import AutoDiagonalNormal
    n, rows, d = 30, 70, 4
    X, y, _, _ = LR.inputs(family, 1, rows, d, True, seed=41)
    model = make_model(family, d, True)
    guide = AutoDiagonalNormal(model)
    params = {k: torch.tensor(v) for k, v in P.logreg_params(guide, d, True, np.random.default_rng(12)).items()}
    params["auto_loc"] = 0.2 * params["auto_loc"]                 # (keeps the Poisson rates moderate)
    Xt, yt, key = torch.tensor(X).cuda(), torch.tensor(y).cuda(), P.key(77)
    draws = PS.posterior_predictive_samples(key, n, model, (Xt,), guide, params)
    want = CR.loo(model, {"w": draws["w"], "intercept": draws["intercept"]}, Xt, yt, pointwise=True)
    got = CR.posterior_loo(key, n, model, (Xt, yt, rows), guide, params, pointwise=True)
    assert got.n_draws == n and got.n_rows == rows and bool(torch.isfinite(got.pointwise["elpd_loo"]).all())
    assert bool(torch.isfinite(got.pointwise["pareto_k"]).all())   # (n = 30: M = 6, a fit in every row)
    _same_bits(got, want)
    w = CR.posterior_waic(key, n, model, (Xt, yt, rows), guide, params, pointwise=True)
    slack = LR.LPPD_EXTRA * np.maximum(1.0, np.abs(np_(w.pointwise["lppd"]).astype(np.float64)))
    assert np.all(np.abs(np_(got.pointwise["lppd"]).astype(np.float64) - np_(w.pointwise["lppd"])) <= slack)   # the same latents
    other = CR.posterior_loo(P.key(78), n, model, (Xt, yt), guide, params, pointwise=True)
    assert not torch.equal(other.pointwise["elpd_loo"], got.pointwise["elpd_loo"])


def test_posterior_loo_mixture_draws_the_latents_of_the_predictive(CR):
    from d3p_amd import mixture as MX
    m, g = _mg()
    k, d, rows, n = 3, 2, MR.T + 5, 30
    obs = MR.soft_inputs(k, d, rows, 1)[0]
    params, args, key = R.posterior_params(k, d, 5), (k, obs, rows, d), R.key(31)
    samples = MX.posterior_predictive_samples(key, n, m, args, g, params)
    want = CR.loo(m, {name: samples[name] for name in ("pis", "mus", "sigs")}, obs, pointwise=True)
    got = CR.posterior_loo(key, n, m, args, g, params, pointwise=True)
    assert got.n_draws == n and got.n_rows == rows
    _same_bits(got, want)
    _same_bits(CR.posterior_loo(key, n, m, (k, None), g, params, pointwise=True, obs=obs, slab_bytes=1), want)


# ---------------------------------------------------------------- compare
def test_compare_on_two_loo_results(CR):
    from d3p_amd.models import LinearRegression, PoissonRegression
    n, rows, d = 31, 129, 33
    X, y, W, b = LR.inputs("poisson", n, rows, d, True)
    Xt, yt, s = torch.tensor(X).cuda(), torch.tensor(y).cuda(), samples_of(W, b)
    a = CR.loo(PoissonRegression(d, intercept=True), s, Xt, yt, pointwise=True)
    lin = CR.loo(LinearRegression(d, intercept=True, obs_scale=LR.SIGMA["linear"]), s, Xt, yt, pointwise=True)
    got = CR.compare(a, lin)
    assert got.elpd_diff.is_cuda and got.elpd_diff.dtype == torch.float64 and got.se_diff.dim() == 0
    diff = np_(a.pointwise["elpd_loo"]).astype(np.float64) - np_(lin.pointwise["elpd_loo"]).astype(np.float64)
    terms = rows * (diff - diff.mean()) ** 2 / (rows - 1)
    tol = rows * 2.0 ** -52
    assert abs(float(got.elpd_diff) - diff.sum()) <= tol * np.abs(diff).sum()
    assert abs(float(got.se_diff) ** 2 - terms.sum()) <= (tol + 2.0 ** -50) * terms.sum()
    assert float(got.se_diff) > 0.0 and float(CR.compare(lin, a).elpd_diff) == -float(got.elpd_diff)
    w = CR.waic(PoissonRegression(d, intercept=True), s, Xt, yt, pointwise=True)
    for pair in ((a, w), (w, lin)):
        with pytest.raises(ValueError, match="of a kind"):
            CR.compare(*pair)
    with pytest.raises(ValueError, match="pointwise"):
        CR.compare(a, CR.loo(PoissonRegression(d, intercept=True), s, Xt, yt))


# ---------------------------------------------------------------- examples
def _example(name):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ex_loo_" + name, os.path.join(root, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_poisson_example_reports_loo_behind_its_flag(CR, capsys):
    import argparse
    import re
    mod = _example("poisson_regression")
    args = argparse.Namespace(sigma=0.5, clip_threshold=1.0, num_steps=300, learning_rate=2e-2, batch_size=200, dimensions=4, num_samples=2000,
                              loo=True, posterior_draws=30)
    mod.main(args)
    out = capsys.readouterr().out
    num = r"(-?[\d.]+)"
    lines = [re.search(name + r" PSIS-LOO \(2000 rows, 30 posterior draws\): elpd_loo " + num + r" \+- " + num + r", p_loo " + num +
                       r", pareto k above " + num + r" in (\d+) rows", out) for name in ("Poisson", "linear")]
    diff = re.search(r"Poisson against linear on the same counts \(PSIS-LOO\): elpd_diff " + num + r" \+- " + num, out)
    assert all(lines) and diff and "WAIC" not in out
    values = [float(v) for m in lines for v in m.groups()] + [float(v) for v in diff.groups()]
    assert np.isfinite(values).all() and abs(values[10] - (values[0] - values[5])) <= 0.02   # (two decimals are printed)


def test_mixture_example_reports_loo_behind_its_flag(CR, capsys):
    import re
    mod = _example("gaussian_mixture_model")
    assert mod.parse_args([]).loo is False                                     # off by default
    mod.main(mod.parse_args("--sigma 1.0 -N 512 -n 2 --loo --posterior-draws 30".split()))
    out = capsys.readouterr().out
    m = re.search(r"PSIS-LOO \(512 points, 30 posterior draws\): elpd_loo (-?[\d.]+) \+- ([\d.]+), p_loo (-?[\d.]+), "
                  r"pareto k above (-?[\d.]+) in (\d+) points", out)
    assert m and np.isfinite([float(v) for v in m.groups()]).all() and "WAIC" not in out
