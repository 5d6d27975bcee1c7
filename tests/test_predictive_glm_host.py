"""d3p_amd.predictive (predictive sampling for the regression family), host side: the module and its C entry point exist, every
validation error is raised before a device is touched, unsupported models and guides are refused -- and the self-checks of
tests/predictive_glm_ref.py, the comparator every test of tests/test_gpu_predictive_glm.py rests on."""
import os
import re

import numpy as np
import pytest
import torch

from . import predictive_glm_ref as G
from .predictive_ref import assert_not_vacuous, key_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("predictive reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


def test_module_exports_exactly_the_three_functions():
    import d3p_amd
    from d3p_amd import predictive as Ps
    assert d3p_amd.predictive is Ps and "predictive" in d3p_amd.__all__
    assert Ps.__all__ == ["predictive_samples", "posterior_predictive_samples", "prior_predictive_samples"]
    for name in Ps.__all__:
        assert "obs" in getattr(Ps, name).__doc__, name
    from d3p_amd import infer_util as U
    from d3p_amd import modelling as M
    from d3p_amd import prediction as Pm
    assert Pm.__all__ == ["predictive_moments", "posterior_predictive_moments"]                                 # (untouched)
    assert U.__all__ == ["log_likelihood", "log_predictive_density", "posterior_log_predictive_density"]
    assert M.__all__ == ["sample_prior_predictive", "sample_posterior_predictive", "sample_multi_prior_predictive",
                         "sample_multi_posterior_predictive", "site_plan", "Site"]


def test_header_and_binding_declare_the_entry_point():
    import d3p_amd._lib as L
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define D3P_ABI_VERSION 9\b", header)
    assert re.search(r"\bint d3p_predict_glm\(void\* stream, const d3p_logreg_model\* model, const float\* X_dev, uint64_t rows, int32_t d,", header)
    res, args = L.SIGNATURES["d3p_predict_glm"]
    assert res is L.C.c_int and len(args) == 12
    assert os.path.join(os.path.dirname(L.__file__), "csrc", "d3p_predict_glm.hip") in L._SRC
    lib = L.load()
    assert lib.d3p_abi_version() == 9
    assert lib.d3p_predict_glm.argtypes == args and lib.d3p_predict_glm.restype is L.C.c_int


def test_predictive_samples_validate_before_the_device(no_device):
    from d3p_amd import predictive as Ps
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    f = Ps.predictive_samples
    X, y = torch.zeros(5, 3), torch.zeros(5)
    w, b = torch.zeros(4, 3), torch.zeros(4)
    plain, icpt = PoissonRegression(3), LinearRegression(3, intercept=True)
    with pytest.raises(ValueError, match="'w' is missing"):
        f(None, plain, {}, X)
    with pytest.raises(ValueError, match=r"posterior_samples\['w'\]"):
        f(None, plain, {"w": torch.zeros(4, 2)}, X)
    with pytest.raises(ValueError, match=r"posterior_samples\['w'\]"):
        f(None, plain, {"w": torch.zeros(0, 3)}, X)
    with pytest.raises(ValueError, match="'intercept' is missing"):
        f(None, icpt, {"w": w}, X)
    with pytest.raises(ValueError, match=r"posterior_samples\['intercept'\]"):
        f(None, icpt, {"w": w, "intercept": torch.zeros(3)}, X)
    with pytest.raises(ValueError, match="2-D"):
        f(None, plain, {"w": w}, torch.zeros(5))
    with pytest.raises(ValueError, match="model_args"):
        f(None, plain, {"w": w})
    with pytest.raises(ValueError, match="columns"):
        f(None, PoissonRegression(4), {"w": w}, X)
    with pytest.raises(NotImplementedError, match="num_obs_total = 9 differs from the 5 rows"):
        f(None, plain, {"w": w}, X, y, 9)
    with pytest.raises(NotImplementedError, match="num_obs_total = 9"):
        f(None, plain, {"w": w}, X, num_obs_total=9)
    # what passes every check arrives at the key, the last check before the device: y and N are accepted and not read
    for model, samples, args in ((plain, {"w": w}, (X,)), (plain, {"w": w}, (X, y)), (plain, {"w": w}, (X, y, 5)), (plain, {"w": w}, (X, None, 5)),
                                 (plain, {"w": w}, (X, torch.zeros(2))), (icpt, {"w": w, "intercept": b.reshape(4, 1)}, (X,)),
                                 (LogisticRegression(3), {"w": np.zeros(3, np.float32)}, (X,)),
                                 (PoissonRegression(3, validate_args=True), {"w": w}, (X, torch.full((5,), 0.5)))):
        with pytest.raises(TypeError, match="rng_key"):
            f(None, model, samples, *args)


def test_posterior_and_prior_samples_validate_before_the_device(no_device):
    from d3p_amd import predictive as Ps
    from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, LinearRegression, LogisticRegression, MeanFieldGuide,
                                PoissonRegression, VAEGuide, VAEModel)
    f, g = Ps.posterior_predictive_samples, Ps.prior_predictive_samples
    X = torch.zeros(5, 3)
    lin, poi, logi = LinearRegression(3, intercept=True), PoissonRegression(3, intercept=True), LogisticRegression(3, intercept=True)
    auto = {"auto_loc": torch.zeros(4), "auto_scale": torch.ones(4)}
    with pytest.raises(ValueError, match="'auto_scale' is missing"):
        f(None, 4, lin, (X,), AutoDiagonalNormal(lin), {"auto_loc": torch.zeros(4)})
    with pytest.raises(ValueError, match="4 values expected"):
        f(None, 4, poi, (X,), AutoDiagonalNormal(poi), {"auto_loc": torch.zeros(3), "auto_scale": torch.ones(4)})
    with pytest.raises(ValueError, match="params"):
        f(None, 4, lin, (X,), AutoDiagonalNormal(lin), None)
    with pytest.raises(ValueError, match="'w_std_log' is missing"):
        f(None, 4, lin, (X,), DiagonalNormalGuide(lin), {"w_loc": torch.zeros(4)})
    for call in (lambda n: f(None, n, lin, (X,), AutoDiagonalNormal(lin), auto), lambda n: g(None, n, poi, (X,))):
        with pytest.raises(ValueError, match="n must be >= 1"):
            call(0)
        with pytest.raises(ValueError, match="n must be >= 1"):
            call(-3)
    with pytest.raises(ValueError, match="model_args"):
        f(None, 4, lin, (), AutoDiagonalNormal(lin), auto)
    with pytest.raises(ValueError, match="model_args"):
        g(None, 4, lin, ())
    with pytest.raises(ValueError, match="2-D"):
        g(None, 4, poi, (torch.zeros(5),))
    with pytest.raises(ValueError, match="columns"):
        f(None, 4, LinearRegression(4, intercept=True), (X,), AutoDiagonalNormal(lin), auto)
    with pytest.raises(NotImplementedError, match="num_obs_total = 7"):
        f(None, 4, lin, (X, None, 7), AutoDiagonalNormal(lin), auto)
    with pytest.raises(NotImplementedError, match="num_obs_total = 7"):
        g(None, 4, poi, (X,), num_obs_total=7)
    for model in (lin, poi):      # the two-site guide is built for logistic regression only
        with pytest.raises(TypeError, match="MeanFieldGuide is not supported"):
            f(None, 4, model, (X,), MeanFieldGuide(model), {})
    with pytest.raises(TypeError, match="VAEGuide is not supported"):
        f(None, 4, logi, (X,), VAEGuide(VAEModel(2, 3)), {})
    with pytest.raises(ValueError, match="'w_loc' is missing"):
        f(None, 4, logi, (X,), MeanFieldGuide(logi), {})
    with pytest.raises(ValueError, match="'mu' is not a sample site of PoissonRegression"):
        g(None, 4, poi, (X,), {"mu": torch.zeros(3)})
    with pytest.raises(ValueError, match=r"substitutes\['w'\]: 3 values expected, got 2"):
        g(None, 4, lin, (X,), {"w": torch.zeros(2)})
    for model in (lin, poi, logi):      # (the key is the last of the checks, still before the device)
        with pytest.raises(TypeError, match="rng_key"):
            f(None, 4, model, (X, torch.zeros(5), 5), AutoDiagonalNormal(model), auto)
        with pytest.raises(TypeError, match="rng_key"):
            g(None, 4, model, (X,), {"w": torch.zeros(3)})


def test_unsupported_models_raise_type_error(no_device):
    from d3p_amd import predictive as Ps
    from d3p_amd.models import AutoDiagonalNormal, GaussianMean, GaussianMixtureModel, VAEModel
    X = torch.zeros(5, 3)
    for model in (GaussianMean(3), GaussianMixtureModel(2, 3), VAEModel(2, 4)):
        for call in (lambda: Ps.predictive_samples(None, model, {"w": torch.zeros(2, 3)}, X),
                     lambda: Ps.posterior_predictive_samples(None, 2, model, (X,), AutoDiagonalNormal(model), {}),
                     lambda: Ps.prior_predictive_samples(None, 2, model, (X,))):
            with pytest.raises(TypeError, match="predictive sampling: unsupported model " + type(model).__name__):
                call()


# ---------------------------------------------------------------- the comparator
@pytest.mark.parametrize("lam", [0.5, 3.0, 9.9, 10.0, 10.5, 50.0, 1e3, 8192.0, 1e6])
def test_restated_rule_is_poisson_distributed(lam):
    """The restatement against scipy.stats.poisson over N = 200 000 outcomes on grid uniforms from a fixed seed: mean and variance within
    5 standard errors, and a chi-square over at most 40 bins of expected count >= 5 N / 40 ... with a p-value above 1e-6."""
    from scipy import stats
    N = 200000
    rng = np.random.default_rng(int(lam * 10) + 1)
    k, _, stable, iters = G.poisson_rule(np.full((1, 1, N), lam), G.GridUniforms(rng, (1, N)))
    k = k[0, 0]
    print(f"lam = {lam}: mean {k.mean()}, var {k.var(ddof=1)}, {iters} iterations at most")
    assert iters <= 16 and k.min() >= 0
    b_mean, b_var = G.poisson_moment_bounds(lam, N)
    assert abs(k.mean() - lam) <= b_mean and abs(k.var(ddof=1) - lam) <= b_var
    edges = np.unique(stats.poisson.ppf(np.linspace(0, 1, 41)[1:-1], lam))          # bins (-inf, e0], (e0, e1], .., (e_last, inf)
    counts = np.bincount(np.searchsorted(edges, k, side="left"), minlength=len(edges) + 1)
    cdf = np.concatenate([[0.0], stats.poisson.cdf(edges, lam), [1.0]])
    expected = N * np.diff(cdf)
    keep = expected > 0
    assert expected[keep].min() >= 5
    chi2 = float(((counts[keep] - expected[keep]) ** 2 / expected[keep]).sum())
    assert counts[~keep].sum() == 0
    assert chi2 <= stats.chi2.ppf(1 - 1e-6, keep.sum() - 1), (lam, chi2)


def test_rule_special_values_and_caps():
    k, sig, _, _ = G.poisson_rule(np.array([np.nan, 0.0, np.inf, 1e-35, 3e9, 1e30]).reshape(1, 1, 6),
                                  G.GridUniforms(np.random.default_rng(0), (1, 6)))
    assert k[0, 0].tolist() == [-1, 0, G.INT_MAX, 0, G.INT_MAX, G.INT_MAX]
    pts = G.lam_interval(np.array([-np.inf, -80.0, 0.0, 88.0, 89.0, 200.0, np.nan]), 0.0)
    assert pts[1].tolist()[:3] == [0.0, 0.0, 1.0] and np.isfinite(pts[:, 3]).all() and np.isposinf(pts[:, 4:6]).all() and np.isnan(pts[:, 6]).all()

    from scipy import stats

    class Never:      # U = 1 - 2^-23 and V = 1: the inversion walks to the largest quantile a grid uniform reaches, PTRS rejects 64 times
        def __call__(self, j, draws=None):
            return np.full((1, 2), 1 - 2.0 ** -23), np.full((1, 2), 1.0)
    k, _, _, iters = G.poisson_rule(np.array([9.5, 40.25]).reshape(1, 1, 2), Never())
    assert k[0, 0].tolist() == [int(stats.poisson.ppf(1 - 2.0 ** -23, 9.5)), 40] and k[0, 0, 0] < 64 and iters == 64


def test_exact_rate_problem_is_exact_in_float32_in_any_order():
    X, w, t = G.exact_rate_problem()
    assert X.shape[0] == 3 * len(G.EXACT_RATES) and np.allclose(np.exp(t[::3]), G.EXACT_RATES, rtol=1e-5)
    lam = np.exp(t[::3])
    assert lam[2] < 10 < lam[3] and abs(lam[2] - 9.99) < 1e-3 and abs(lam[3] - 10.01) < 1e-3
    rng = np.random.default_rng(3)
    for _ in range(20):
        order = rng.permutation(X.shape[1])
        acc = np.zeros(X.shape[0], np.float32)
        for c in order:
            acc = (acc + X[:, c] * w[c]).astype(np.float32)
        assert np.array_equal(acc.astype(np.float64), t)


def test_unjudged_share_of_the_gpu_inputs_with_a_float32_lam(O):
    """The calibration of the comparator's margins: the device replaced by numpy's float32 matmul and exp on the GPU tests' inputs.
    Every judged outcome is equal and the unjudged share stays under the vacuity cap."""
    for d, rows, n, intercept in G.TILE_EDGES:
        seed = G.edge_seed(d, rows, n, intercept)
        X, params = G.generic_problem(d, rows, n, intercept, seed)
        w, b, okeys = G.oracle_draws(O, key_words(seed), n, d, intercept, params, rows)
        t, _ = G.linear_predictor(X, w, b, d)
        assert -3.1 <= t.min() and t.max() <= 4.0
        sim = G.simulated_device_poisson(O, X, w, b, okeys, d)
        share = G.check_poisson(O, sim, X, w, b, okeys, d, f"simulated d={d} rows={rows} n={n} intercept={intercept}")
        print(f"d={d} rows={rows} n={n} intercept={intercept}: unjudged {share:.5f} of {n * rows}")
        assert_not_vacuous(share, n * rows)
    X, wv, t = G.exact_rate_problem()
    n, d = 256, X.shape[1]
    w, b, okeys = G.oracle_draws(O, key_words(77), n, d, False, None, X.shape[0], posterior=False, subst={"w": wv})
    sim = G.simulated_device_poisson(O, X, w, None, okeys, d)
    assert np.array_equal((w.astype(np.float32) @ X.T).astype(np.float64), np.broadcast_to(t, (n, len(t))))
    for i, rate in enumerate(G.EXACT_RATES):       # per rate: the cap holds at each, not only on average
        rws = slice(3 * i, 3 * i + 3)
        exp, judged, iters = G.judge_poisson(np.broadcast_to(t[rws], (n, 3)), 0.0, _RowsOf(G.ObsUniforms(O, okeys, X.shape[0]), rws))
        assert np.array_equal(sim[:, rws][judged], exp[judged])
        share = float((~judged).mean())
        print(f"rate {rate}: unjudged {share:.5f} of {n * 3}, {iters} iterations at most, mean outcome {sim[:, rws].mean():.3f}")
        assert_not_vacuous(share, n * 3)
    share = G.check_poisson(O, sim, X, w, None, okeys, d, "simulated exact rates", exact=True)
    assert_not_vacuous(share, sim.size)


class _RowsOf:
    """A row slice of a uniform source."""

    def __init__(self, unif, rows):
        self.unif, self.rows = unif, rows

    def __call__(self, j, draws=None):
        U, V = self.unif(j, draws)
        return U[:, self.rows], V[:, self.rows]


def test_linear_bound_tells_a_fused_multiply_add_free_result_from_a_wrong_one(O):
    """check_linear passes the float32 two-rounding result of the oracle's eps and refuses one whose noise is scaled by 1 + 2^-10."""
    d, rows, n, intercept = 33, 129, 5, True
    X, params = G.generic_problem(d, rows, n, intercept, 11)
    w, b, okeys = G.oracle_draws(O, key_words(11), n, d, intercept, params, rows)
    t32 = (w @ X.T + b[:, None]).astype(np.float32)
    eps = np.stack([O.tf_normal(k, rows) for k in okeys])
    sigma = np.float32(0.75)
    good = (t32 + (eps * sigma).astype(np.float32)).astype(np.float32)
    G.check_linear(O, good, X, w, b, float(sigma), okeys, d, "two roundings")
    with pytest.raises(AssertionError, match="max err"):
        G.check_linear(O, (t32 + eps * sigma * np.float32(1 + 2.0 ** -10)).astype(np.float32), X, w, b, float(sigma), okeys, d, "scaled")
    with pytest.raises(AssertionError, match="max err"):
        G.check_linear(O, np.roll(good, 1, axis=1), X, w, b, float(sigma), okeys, d, "shifted rows")
