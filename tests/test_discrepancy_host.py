"""d3p_amd.discrepancy (realized-discrepancy checks and the Bayesian R^2), host side: the module and its C entries exist, every refusal
is raised before a device is touched, the derived values are right on small matrices -- and the self-checks of
tests/discrepancy_ref.py, the restatement every comparison of tests/test_gpu_discrepancy.py rests on."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from . import discrepancy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 0.75


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("discrepancy reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


def _small(family, n, rows, seed):
    """mu (float32), v and y as the kernels would hold them, from numpy's samplers."""
    rng = np.random.default_rng(seed)
    t = rng.normal(size=(n, rows)).astype(np.float32)
    if family == "linear":
        mu = t
        v = (mu + SIGMA * rng.normal(size=(n, rows))).astype(np.float32)
        y = (mu[0] + rng.normal(size=rows)).astype(np.float32)
    elif family == "poisson":
        mu = np.exp(t + np.float32(1.0)).astype(np.float32)
        v = rng.poisson(mu).astype(np.int32)
        y = rng.poisson(mu[0] * 1.5).astype(np.float32)
    else:
        mu = (1.0 / (1.0 + np.exp(-t.astype(np.float64)))).astype(np.float32)
        v = (rng.random(size=(n, rows)) < mu).astype(np.int32)
        y = (rng.random(size=rows) < 0.4).astype(np.float32)
    return mu, v, y


# ------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("rows", [1, 33, 129, 300, 1000])
def test_restatement_lies_within_the_order_bound_of_fsum(family, rows):
    """Any order of adding `rows` float64 terms differs from the exact sum by at most (rows - 1) u sum|term| (1 + O(rows u)), u =
    2^-53 (Higham, Accuracy and Stability, eq. 4.4); fsum rounds the exact sum once more (u |sum| <= u sum|term|): rows 2^-53 sum|term|."""
    mu, v, y = _small(family, 3, rows, rows)
    for shift in (0.0, 1.25, float(np.float32(y.mean()))):
        got = R.discrepancy(family, mu, v, y, shift, SIGMA)
        ref = R.discrepancy_naive(family, mu, v, y, shift, SIGMA)
        bound = rows * 2.0 ** -53 * np.abs(R.terms(family, mu, v, y, shift, SIGMA)).sum(axis=2)
        assert got.shape == ref.shape == (6, 3) and np.isfinite(got).all()
        assert np.all(np.abs(got - ref) <= bound), (family, rows, shift)
    # a draw's sums do not depend on the other draws
    assert R.same(R.discrepancy(family, mu[1], v[1], y, 0.5, SIGMA)[:, 0], R.discrepancy(family, mu, v, y, 0.5, SIGMA)[:, 1])


def test_restatement_on_integers_is_exact():
    """Poisson with integral means: every term of outputs 2 to 5 and every partial sum is an integer."""
    rng = np.random.default_rng(2)
    mu = rng.integers(1, 9, size=(2, 300)).astype(np.float32)
    v = rng.integers(0, 20, size=(2, 300)).astype(np.int32)
    y = rng.integers(0, 20, size=300).astype(np.float32)
    got = R.discrepancy("poisson", mu, v, y, 3.0)
    m, ey = mu.astype(np.int64) - 3, y.astype(np.int64)[None] - mu.astype(np.int64)
    assert np.array_equal(got[2], m.sum(1)) and np.array_equal(got[3], (m * m).sum(1))
    assert np.array_equal(got[4], ey.sum(1)) and np.array_equal(got[5], (ey * ey).sum(1))


def test_conventions_of_q():
    f32, i32 = np.float32, np.int32
    # Poisson, mu == 0: a matched row gives 0, a count of 1 gives +inf; a NaN mean gives NaN -- in its own draw only
    mu = np.array([[0.0, 0.0, 2.0], [np.nan, 1.0, 2.0], [1.0, 1.0, 2.0]], f32)
    v = np.array([[0, 0, 2], [-1, 1, 3], [0, 1, 2]], i32)
    t = R.terms("poisson", mu, v, np.array([0.0, 1.0, 2.0], f32), 0.0)
    assert t[0, 0].tolist() == [0.0, np.inf, 0.0] and t[1, 0].tolist() == [0.0, 0.0, 0.0]
    assert np.isnan(t[:, 1, 0]).all() and t[0, 1, 1:].tolist() == [0.0, 0.0] and t[1, 1, 2] == 0.5
    s = R.discrepancy("poisson", mu, v, np.array([0.0, 1.0, 2.0], f32), 0.0)
    assert s[0, 0] == np.inf and s[1, 0] == 0.0 and np.isnan(s[:, 1]).all() and np.isfinite(s[:, 2]).all()
    assert s[:, 2].tolist() == [1.0, 1.0, 4.0, 6.0, -1.0, 1.0]
    # logistic, mu exactly 0 and 1 (V == 0 on both sides): matched 0, mismatched +inf
    mu = np.array([[0.0, 0.0, 1.0, 1.0, 0.5]], f32)
    t = R.terms("logistic", mu, np.array([[0, 1, 1, 0, 1]], i32), np.array([1.0, 0.0, 0.0, 1.0, 0.0], f32), 0.0)
    assert t[0, 0].tolist() == [np.inf, 0.0, np.inf, 0.0, 1.0] and t[1, 0].tolist() == [0.0, np.inf, 0.0, np.inf, 1.0]
    # linear: V = fl64(float32(sigma))^2 whatever mu is; nothing is matched specially but e == 0
    t = R.terms("linear", np.array([[1.0, 2.0]], f32), np.array([[1.0, 3.5]], f32), np.array([0.0, 2.0], f32), 0.0, 0.1)
    s2 = np.float64(f32(0.1)) ** 2
    assert t[0, 0].tolist() == [1.0 / s2, 0.0] and t[1, 0].tolist() == [0.0, 2.25 / s2]


# ------------------------------------------------------------------------------- the derived values
@pytest.mark.parametrize("family", R.FAMILIES)
def test_derived_values_and_both_r2_kinds_against_direct_formulas(family):
    from d3p_amd import discrepancy as D
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    n, rows = 4, 37
    mu, v, y = _small(family, n, rows, 5)
    shift = float(np.float32(y.mean()))
    six = R.discrepancy(family, mu, v, y, shift, SIGMA)
    model = {"linear": LinearRegression(3, obs_scale=SIGMA), "poisson": PoissonRegression(3), "logistic": LogisticRegression(3)}[family]
    M = mu.astype(np.float64)
    for wrap in (lambda a: a, lambda a: torch.tensor(a, dtype=torch.float64)):
        s = D.DiscrepancySums(*(wrap(a) for a in six), rows, shift)
        val = lambda x: np.asarray(x, np.float64)
        mean_mu = shift + six[2] / rows
        var_fit = (six[3] - six[2] * six[2] / rows) / (rows - 1)
        var_res = (six[5] - six[4] * six[4] / rows) / (rows - 1)
        assert np.array_equal(val(s.mean_mu), mean_mu)
        assert np.array_equal(val(s.var_fit()), var_fit) and np.array_equal(val(s.var_fit(ddof=0)), (six[3] - six[2] * six[2] / rows) / rows)
        assert np.array_equal(val(s.var_res()), var_res)
        assert np.array_equal(val(s.bias), six[4] / rows) and np.array_equal(val(s.rmse), np.sqrt(six[5] / rows))
        assert np.array_equal(val(s.dispersion), six[0] / rows)
        assert np.array_equal(val(s.bayes_r2("residual")), var_fit / (var_fit + var_res))
        if family == "linear":
            expect = np.float64(np.float32(SIGMA)) ** 2
        elif family == "poisson":
            expect = mean_mu
        else:
            expect = mean_mu - (six[3] / rows + (2.0 * (mean_mu - shift)) * shift + shift * shift)
        assert np.array_equal(np.broadcast_to(val(s.expected_var_res(model)), (n,)), np.broadcast_to(expect, (n,)))
        assert np.array_equal(val(s.bayes_r2("model", model)), var_fit / (var_fit + expect))
        with pytest.raises(ValueError, match="model is required"):
            s.bayes_r2("model")
        s.model = model
        assert np.array_equal(val(s.bayes_r2("model")), var_fit / (var_fit + expect))
        with pytest.raises(ValueError, match="unknown R\\^2 kind"):
            s.bayes_r2("adjusted")
        for kind in D.R2_KINDS:
            r2 = val(s.bayes_r2(kind))
            assert np.all((r2 >= 0.0) & (r2 <= 1.0)), (family, kind)
        # ... and the direct formulas are what they say, up to the cancellation the shift is there to avoid
        assert np.allclose(val(s.mean_mu), M.mean(1), rtol=1e-12) and np.allclose(val(s.var_fit()), M.var(1, ddof=1), rtol=1e-10)
        res = y.astype(np.float64)[None] - M
        assert np.allclose(val(s.var_res()), res.var(1, ddof=1), rtol=1e-10) and np.allclose(val(s.rmse), np.sqrt((res * res).mean(1)), rtol=1e-12)
        if family == "logistic":
            assert np.allclose(val(s.expected_var_res()), (M * (1.0 - M)).mean(1), rtol=1e-10)
    one = D.DiscrepancySums(*(torch.tensor([0.0], dtype=torch.float64) for _ in range(6)), 1, 2.0)
    assert math.isnan(float(one.var_fit()[0])) and float(one.var_fit(ddof=0)[0]) == 0.0 and float(one.mean_mu[0]) == 2.0


def test_paired_tail_shares_and_result_lines():
    from d3p_amd import discrepancy as D
    obs = np.array([1.0, 5.0, 2.0, np.nan, 3.0])
    rep = np.array([2.0, 4.0, 2.0, 1.0, np.nan])
    assert D._paired_tail_shares(rep, obs) == (0.4, 0.4)             # paired per draw; the tie counts twice, a NaN on neither side
    assert D._paired_tail_shares(np.array([np.inf, 1.0]), np.array([np.inf, 0.0])) == (1.0, 0.5)
    r2 = {"residual": np.array([0.5, 0.6]), "model": np.array([0.4, np.nan])}
    res = D.DiscrepancyResult(np.array([8.0, 9.0]), np.array([1.0, np.inf]), 0.5, 0.5, np.array([4.0, 4.5]), r2, np.ones(2), np.zeros(2), 2, 2, 1)
    lines = res.lines()
    assert lines[0].startswith("discrepancy chi2") and "p_ge 0.500" in lines[0] and "1 not finite" in lines[0]
    assert [l.split()[1] for l in lines[1:]] == ["chi2_obs", "chi2_rep", "dispersion", "r2_residual", "r2_model", "rmse", "bias"]


# ------------------------------------------------------------------------------- the C boundary without a device
def test_header_and_binding_declare_the_two_symbols():
    import d3p_amd._lib as L
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    assert re.search(r"\bsize_t d3p_predict_discrepancy_workspace\(uint64_t rows, uint32_t n\);", hdr)
    assert re.search(r"\bint d3p_predict_discrepancy\(void\* stream, const d3p_logreg_model\* model, const float\* X_dev, const float\* y_dev, "
                     r"uint64_t rows, int32_t d,", hdr)
    arity = {"d3p_predict_discrepancy_workspace": 2, "d3p_predict_discrepancy": 16}
    for name, n in arity.items():
        args = re.search(r"\b" + name + r"\(([^)]*)\);", hdr).group(1)
        assert args.count(",") + 1 == n == len(L.SIGNATURES[name][1]), name
    assert L.SIGNATURES["d3p_predict_discrepancy_workspace"][0] is L.C.c_size_t and L.SIGNATURES["d3p_predict_discrepancy"][0] is L.C.c_int
    assert L.SIGNATURES["d3p_predict_discrepancy"][1][12] is L.C.c_double
    csrc = os.path.join(os.path.dirname(L.__file__), "csrc")
    assert os.path.join(csrc, "d3p_discrepancy.hip") in L._SRC and os.path.join(csrc, "d3p_discrepancy.hip") in L._DEPS
    lib = L.load()
    assert lib.d3p_abi_version() == 9
    for name in arity:
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]


def test_workspace_size_follows_the_strip_function():
    import d3p_amd._lib as L
    lib = L.load()
    for rows, n in ((1, 1), (128, 7), (129, 128), (65536, 3), (65537, 3), (10 ** 6, 128)):
        assert lib.d3p_predict_discrepancy_workspace(rows, n) == R.strips(rows)[2] * 6 * n * 8
    assert R.strips(65537) == (513, 2, 257) and R.strips(10 ** 6) == (7813, 16, 489)
    assert lib.d3p_predict_discrepancy_workspace(0, 4) == 0 and lib.d3p_predict_discrepancy_workspace(2 ** 32, 4) == 0


def test_c_refusals_that_need_no_device():
    """The argument errors of d3p_predict_discrepancy that are decided before any pointer is examined on a device."""
    import d3p_amd._lib as L
    lib = L.load()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    d = 3

    def call(ms, X=p, y=p, rows=5, d_=d, lat=p, ld=d + 1, w_off=0, b_col=-1, n=2, keys=p, shift=0.0, out=p, ws=p, nb=512):
        return lib.d3p_predict_discrepancy(None, L.C.byref(ms) if ms is not None else None, X, y, rows, d_, lat, ld, w_off, b_col, n, keys, shift,
                                           out, ws, nb)

    model = lambda fam, intercept=0, guide=L.D3P_GUIDE_SOFTPLUS, sigma=1.0: L.LogregModel(d, intercept, 1.0, 1.0, 1.0, 1.0, fam, guide, sigma)
    lin, poi, logi = model(L.D3P_FAMILY_LINREG), model(L.D3P_FAMILY_POISSON), model(L.D3P_FAMILY_LOGREG)
    assert call(None) == -1 and b"null model" in lib.d3p_last_error()
    assert call(model(L.D3P_FAMILY_GAUSS_MEAN)) == -3 and b"Gaussian-mean" in lib.d3p_last_error()
    assert call(model(L.D3P_FAMILY_LOGREG, 1, L.D3P_GUIDE_EXP_SITES)) == -3 and b"D3P_GUIDE_EXP_SITES" in lib.d3p_last_error()
    for bad_sigma in (0.0, -1.0, math.inf, math.nan):
        assert call(model(L.D3P_FAMILY_LINREG, sigma=bad_sigma)) == -1 and b"lik_sigma" in lib.d3p_last_error()
    for ms in (lin, poi, logi):
        assert call(ms, y=None) == -1 and b"null" in lib.d3p_last_error()
        assert call(ms, X=None) == -1 and b"null X / y / latent / obs_keys / out pointer" in lib.d3p_last_error()
        assert call(ms, lat=None) == -1 and call(ms, keys=None) == -1 and call(ms, out=None) == -1
        assert call(ms, d_=d + 1) == -1 and b"differs from the model's" in lib.d3p_last_error()
        assert call(ms, n=0) == -1 and b"n must be" in lib.d3p_last_error()
        assert call(ms, ld=d - 1) == -1 and b"latent row" in lib.d3p_last_error()
        assert call(ms, w_off=2) == -1 and call(ms, w_off=-1) == -1
        assert call(ms, b_col=1) == -1 and b"latent row" in lib.d3p_last_error()          # inside the weights
        assert call(ms, b_col=d) == -1 and b"exactly when the model has an intercept" in lib.d3p_last_error()
        assert call(ms, rows=2 ** 32) == -1 and call(ms, n=128 * 65535 + 1) == -1
        assert call(ms, rows=0) == -1 and b"rows must be" in lib.d3p_last_error()
    assert call(model(L.D3P_FAMILY_LOGREG, 1)) == -1 and b"exactly when the model has an intercept" in lib.d3p_last_error()
    assert call(poi, rows=2 ** 31) == -1 and b"2 rows < 2^32" in lib.d3p_last_error()
    assert np.all(buf == 0.0)


# ------------------------------------------------------------------------------- the Python layer without a device
def test_module_surface_and_lazy_import():
    import d3p_amd
    from d3p_amd import discrepancy as D
    assert d3p_amd.discrepancy is D and "discrepancy" in d3p_amd.__all__
    assert D.__all__ == ["predictive_discrepancy", "posterior_predictive_discrepancy", "discrepancy_check", "DiscrepancySums",
                         "DiscrepancyResult", "R2_KINDS"]
    assert D.DiscrepancySums._fields == ("chi2_obs", "chi2_rep", "mu_sum", "mu_sumsq", "res_sum", "res_sumsq", "n_rows", "shift")
    assert D.DiscrepancyResult._fields == ("chi2_obs", "chi2_rep", "p_ge", "p_le", "dispersion", "r2", "rmse", "bias", "n_draws", "n_rows",
                                           "n_nonfinite")
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.discrepancy' not in sys.modules; " \
           "d3p_amd.discrepancy; assert 'd3p_amd.discrepancy' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_the_kernel_calls_the_shared_outcome_rules_and_has_no_atomics():
    with open(os.path.join(ROOT, "d3p_amd", "csrc", "d3p_discrepancy.hip")) as f:
        text = f.read()
    with open(os.path.join(ROOT, "d3p_amd", "csrc", "d3p_outcome.h")) as f:
        outcome = f.read()
    choice = outcome[outcome.index("auto glm_outcome("):]   # the one choice among the rules, built on the one definition of each
    for call in ("poisson_draw(", "bernoulli_draw(", "sigmoid_probs(", "normal_site_value(", "tile_product(", "tile_scatter("):
        assert call in text or ("glm_outcome<FAMILY>(" in text and call in choice), call
    for definition in (r"int32_t poisson_draw\(", r"int32_t bernoulli_draw\(", r"float sigmoid_probs\(", r"float normal_site_value\("):
        assert not re.search(definition, text), definition
    assert "atomic" not in text.lower().replace("no floating-point atomics", "")
    assert "#pragma clang fp contract(off)" in text


def test_sampling_refusals_are_kept(no_device):
    from d3p_amd import discrepancy as D
    from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, GaussianMean, GaussianMixtureModel, LinearRegression,
                                LogisticRegression, MeanFieldGuide, PoissonRegression, VAEGuide, VAEModel)
    X, y = torch.zeros(5, 3), torch.zeros(5)
    lin, poi, logi = LinearRegression(3, intercept=True), PoissonRegression(3, intercept=True), LogisticRegression(3, intercept=True)
    auto = {"auto_loc": torch.zeros(4), "auto_scale": torch.ones(4)}
    w = {"w": torch.zeros(4, 3), "intercept": torch.zeros(4)}
    post = (lambda n, model, args, guide, params, **k: D.posterior_predictive_discrepancy(None, n, model, args, guide, params, **k),
            lambda n, model, args, guide, params, **k: D.discrepancy_check(None, n, model, args, guide, params, **k))
    for bad in (GaussianMean(3), GaussianMixtureModel(2, 3), VAEModel(2, 3)):
        with pytest.raises(TypeError, match="unsupported model"):
            D.predictive_discrepancy(None, bad, w, X, y)
        for f in post:
            with pytest.raises(TypeError, match="unsupported model"):
                f(4, bad, (X, y), AutoDiagonalNormal(lin), auto)
    for f in post:
        for model in (lin, poi):
            with pytest.raises(TypeError, match="MeanFieldGuide is not supported"):
                f(4, model, (X, y), MeanFieldGuide(model), {})
        with pytest.raises(TypeError, match="VAEGuide is not supported"):
            f(4, logi, (X, y), VAEGuide(VAEModel(2, 3)), {})
        for n in (0, -2):
            with pytest.raises(ValueError, match="n must be >= 1"):
                f(n, lin, (X, y), AutoDiagonalNormal(lin), auto)
        with pytest.raises(ValueError, match="model_args"):
            f(4, lin, (), AutoDiagonalNormal(lin), auto)
        with pytest.raises(ValueError, match="columns"):
            f(4, LinearRegression(4, intercept=True), (X, y), AutoDiagonalNormal(lin), auto)
        with pytest.raises(NotImplementedError, match="num_obs_total = 7"):
            f(4, lin, (X, y, 7), AutoDiagonalNormal(lin), auto)
        with pytest.raises(ValueError, match="params"):
            f(4, lin, (X, y), AutoDiagonalNormal(lin), None)
        with pytest.raises(ValueError, match="'auto_scale' is missing"):
            f(4, lin, (X, y), AutoDiagonalNormal(lin), {"auto_loc": torch.zeros(4)})
        with pytest.raises(ValueError, match="'w_std_log' is missing"):
            f(4, poi, (X, y), DiagonalNormalGuide(poi), {"w_loc": torch.zeros(4)})
        with pytest.raises(ValueError, match="y is missing"):
            f(4, poi, (X,), AutoDiagonalNormal(poi), auto)
        with pytest.raises(ValueError, match="y is missing"):
            f(4, poi, (X, None), AutoDiagonalNormal(poi), auto)
        with pytest.raises(ValueError, match="5 values expected"):
            f(4, poi, (X, torch.zeros(4)), AutoDiagonalNormal(poi), auto)
        for model in (poi, logi):
            with pytest.raises(ValueError, match="non-integral"):
                f(4, model, (X, torch.tensor([0.0, 1.0, 0.5, 1.0, 0.0])), AutoDiagonalNormal(model), auto)
            with pytest.raises(ValueError, match="non-integral"):
                f(4, model, (X, np.array([0.0, 1.0, np.nan, 1.0, 0.0])), AutoDiagonalNormal(model), auto)
        with pytest.raises(TypeError, match="rng_key"):             # everything passes: the key is the last check before the device
            f(4, poi, (X, y), AutoDiagonalNormal(poi), auto)
        with pytest.raises(TypeError, match="rng_key"):             # any float is an outcome of the linear family
            f(4, lin, (X, torch.tensor([0.0, 1.0, 0.5, 1.0, 0.0])), AutoDiagonalNormal(lin), auto)
        with pytest.raises(TypeError, match="rng_key"):
            f(4, logi, (X, y), MeanFieldGuide(logi), {"w_loc": torch.zeros(3), "w_std_log": torch.zeros(3), "intercept_loc": torch.zeros(1),
                                                      "intercept_std_log": torch.zeros(1)})
    for bad in (math.nan, math.inf):
        with pytest.raises(ValueError, match="finite"):
            D.posterior_predictive_discrepancy(None, 4, lin, (X, y), AutoDiagonalNormal(lin), auto, shift=bad)
        with pytest.raises(ValueError, match="finite"):
            D.predictive_discrepancy(None, lin, w, X, y, shift=bad)
    # predictive_discrepancy: predictive_samples' checks, then y's
    with pytest.raises(ValueError, match="'w' is missing"):
        D.predictive_discrepancy(None, lin, {}, X, y)
    with pytest.raises(ValueError, match="'intercept' is missing"):
        D.predictive_discrepancy(None, lin, {"w": torch.zeros(4, 3)}, X, y)
    with pytest.raises(ValueError, match="2-D"):
        D.predictive_discrepancy(None, lin, w, torch.zeros(5), y)
    with pytest.raises(NotImplementedError, match="num_obs_total = 9"):
        D.predictive_discrepancy(None, lin, w, X, y, 9)
    with pytest.raises(ValueError, match="y is missing"):
        D.predictive_discrepancy(None, lin, w, X)
    with pytest.raises(ValueError, match="non-integral"):
        D.predictive_discrepancy(None, poi, w, X, torch.full((5,), 0.5))
    with pytest.raises(TypeError, match="rng_key"):
        D.predictive_discrepancy(None, lin, w, X, y, shift=1.5)


# ------------------------------------------------------------------------------- what the check means, on the CPU
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_zero_inflation_margin_on_the_cpu(seed):
    """The misfit check of tests/test_gpu_discrepancy.py with numpy's Poisson sampler: 2000 rows at a predictor near 2 (rate e^2 = 7.4),
    50 draws with 1e-3 jitter, every second y set to 0.  A replicate's chi-square is a sum of 2000 terms of mean 1 and variance 2 + 1 /
    7.4 (2000 +- 65); a zeroed row contributes (0 - 7.4)^2 / 7.4 = 7.4, so chi2_obs is near 1000 + 7400.  Over seeds 0 .. 199 of this
    setup the smallest chi2_obs (>= 8272) exceeded the largest chi2_rep (<= 2330) by a factor >= 3.57; asserted: a factor above 2 for
    every seed run."""
    rows, n = 2000, 50
    rng = np.random.default_rng(seed)
    t = (2.0 + 1e-3 * rng.normal(size=(n, rows))).astype(np.float32)
    mu = np.exp(t).astype(np.float32)
    v = rng.poisson(mu).astype(np.int32)
    y = rng.poisson(mu[0]).astype(np.float32)
    y[::2] = 0.0
    six = R.discrepancy("poisson", mu, v, y, float(np.float32(y.mean())))
    assert six[0].min() > 2.0 * six[1].max()
    assert (six[0] / rows).min() > 2.0 and (six[1] / rows).max() < 1.3
