"""d3p_amd.prediction (posterior predictive mean and variance), host side: the module and its C entry point exist, every validation
error is raised before a device is touched, unsupported models and guides are refused -- and the self-checks of
tests/moments_ref.py, the comparator every test of tests/test_gpu_moments.py rests on."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("prediction reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


def test_module_exports_exactly_the_two_functions():
    import d3p_amd
    from d3p_amd import prediction as Pm
    assert d3p_amd.prediction is Pm
    assert Pm.__all__ == ["predictive_moments", "posterior_predictive_moments"]
    for name in Pm.__all__:
        assert "variance" in getattr(Pm, name).__doc__ or "predictive_moments" in getattr(Pm, name).__doc__, name
    from d3p_amd import infer_util as U
    assert U.__all__ == ["log_likelihood", "log_predictive_density", "posterior_log_predictive_density"]      # (untouched)


def test_header_and_binding_declare_the_entry_point():
    import d3p_amd._lib as L
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define D3P_ABI_VERSION 9\b", header)
    assert re.search(r"\bint d3p_predict_moments\(void\* stream, const d3p_logreg_model\* model, const float\* X_dev, uint64_t rows,", header)
    res, args = L.SIGNATURES["d3p_predict_moments"]
    assert res is L.C.c_int and len(args) == 11
    assert os.path.join(os.path.dirname(L.__file__), "csrc", "d3p_moments.hip") in L._SRC
    lib = L.load()
    assert lib.d3p_predict_moments.argtypes == args and lib.d3p_predict_moments.restype is L.C.c_int


def test_validation_comes_before_the_device(no_device):
    from d3p_amd import prediction as Pm
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    f = Pm.predictive_moments
    X, y = torch.zeros(5, 3), torch.zeros(5)
    w, b = torch.zeros(4, 3), torch.zeros(4)
    plain, icpt = LogisticRegression(3), LinearRegression(3, intercept=True)
    with pytest.raises(ValueError, match="'w' is missing"):
        f(plain, {}, X)
    with pytest.raises(ValueError, match="'w' is missing"):
        f(plain, None, X, y)
    with pytest.raises(ValueError, match=r"posterior_samples\['w'\]"):
        f(plain, {"w": torch.zeros(4, 2)}, X)
    with pytest.raises(ValueError, match=r"posterior_samples\['w'\]"):
        f(plain, {"w": np.zeros((2, 4, 3), np.float32)}, X)
    with pytest.raises(ValueError, match=r"posterior_samples\['w'\]"):
        f(plain, {"w": torch.zeros(0, 3)}, X)
    with pytest.raises(ValueError, match="'intercept' is missing"):
        f(icpt, {"w": w}, X)
    with pytest.raises(ValueError, match=r"posterior_samples\['intercept'\]"):
        f(icpt, {"w": w, "intercept": torch.zeros(3)}, X)
    with pytest.raises(ValueError, match="2-D"):
        f(plain, {"w": w}, torch.zeros(5))
    with pytest.raises(ValueError, match="2-D"):
        f(plain, {"w": w}, torch.zeros(5, 3, 1), y)
    with pytest.raises(ValueError, match="model_args"):
        f(plain, {"w": w})
    with pytest.raises(ValueError, match="columns"):
        f(LogisticRegression(4), {"w": w}, X)
    # ... and what passes every check goes on to the device: y and N are accepted and not read, labels are not validated
    half = torch.full((5,), 0.5)
    for model, samples, args in ((plain, {"w": w}, (X,)), (plain, {"w": w}, (X, y)), (plain, {"w": w}, (X, y, 5)), (plain, {"w": w}, (X, None, 5)),
                                 (plain, {"w": w}, (X, torch.zeros(2))), (icpt, {"w": w, "intercept": b.reshape(4, 1)}, (X,)),
                                 (plain, {"w": np.zeros(3, np.float32)}, (X,)), (PoissonRegression(3, validate_args=True), {"w": w}, (X, half))):
        with pytest.raises(AssertionError, match="reached require_device"):
            f(model, samples, *args)


def test_posterior_moments_validate_before_the_device(no_device):
    from d3p_amd import prediction as Pm
    from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, LinearRegression, LogisticRegression, MeanFieldGuide,
                                PoissonRegression, VAEGuide, VAEModel)
    f = Pm.posterior_predictive_moments
    X = torch.zeros(5, 3)
    lin, logi = LinearRegression(3, intercept=True), LogisticRegression(3, intercept=True)
    auto = {"auto_loc": torch.zeros(4), "auto_scale": torch.ones(4)}
    with pytest.raises(ValueError, match="'auto_scale' is missing"):
        f(None, 4, lin, (X,), AutoDiagonalNormal(lin), {"auto_loc": torch.zeros(4)})
    with pytest.raises(ValueError, match="4 values expected"):
        f(None, 4, lin, (X,), AutoDiagonalNormal(lin), {"auto_loc": torch.zeros(3), "auto_scale": torch.ones(4)})
    with pytest.raises(ValueError, match="params"):
        f(None, 4, lin, (X,), AutoDiagonalNormal(lin), None)
    with pytest.raises(ValueError, match="'w_std_log' is missing"):
        f(None, 4, lin, (X,), DiagonalNormalGuide(lin), {"w_loc": torch.zeros(4)})
    with pytest.raises(ValueError, match="n must be >= 1"):
        f(None, 0, lin, (X,), AutoDiagonalNormal(lin), auto)
    with pytest.raises(ValueError, match="model_args"):
        f(None, 4, lin, (), AutoDiagonalNormal(lin), auto)
    with pytest.raises(ValueError, match="2-D"):
        f(None, 4, lin, (torch.zeros(5),), AutoDiagonalNormal(lin), auto)
    with pytest.raises(ValueError, match="columns"):
        f(None, 4, LinearRegression(4, intercept=True), (X,), AutoDiagonalNormal(lin), auto)
    for model in (lin, PoissonRegression(3, intercept=True)):      # the two-site guide is built for logistic regression only
        with pytest.raises(TypeError, match="MeanFieldGuide is not supported"):
            f(None, 4, model, (X,), MeanFieldGuide(model), {})
    with pytest.raises(TypeError, match="VAEGuide is not supported"):
        f(None, 4, logi, (X,), VAEGuide(VAEModel(2, 3)), {})
    with pytest.raises(ValueError, match="'w_loc' is missing"):
        f(None, 4, logi, (X,), MeanFieldGuide(logi), {})
    pm = PoissonRegression(3, intercept=True, validate_args=True)      # labels are not read: check_labels is not called
    for model, args in ((lin, (X,)), (lin, (X, torch.zeros(5), 5)), (pm, (X, torch.full((5,), 0.5)))):
        with pytest.raises(TypeError, match="rng_key"):          # (the key is the last of the checks, still before the device)
            f(None, 4, model, args, AutoDiagonalNormal(model), auto)


def test_unsupported_models_raise_type_error(no_device):
    from d3p_amd import prediction as Pm
    from d3p_amd.models import AutoDiagonalNormal, GaussianMean, GaussianMixtureModel, VAEModel
    X = torch.zeros(5, 3)
    for model in (GaussianMean(3), GaussianMixtureModel(2, 3), VAEModel(2, 4)):
        for call in (lambda: Pm.predictive_moments(model, {"w": torch.zeros(2, 3)}, X),
                     lambda: Pm.posterior_predictive_moments(None, 2, model, (X,), AutoDiagonalNormal(model), {})):
            with pytest.raises(TypeError, match="predictive_moments: unsupported model " + type(model).__name__):
                call()


# ---------------------------------------------------------------- the comparator
def test_comparator_logistic_variance_is_the_law_of_total_variance():
    from tests import moments_ref as MR
    X, _, W, b = MR.LR.inputs("logistic", 37, 50, 9, True)
    t = MR.LR.linear_predictor(X, W, b)
    t[:, :5] *= 6.0                                     # some rows saturate: p near 0 or 1
    mean, var = MR.moments_of_t("logistic", t, 1.0)
    p = MR.P.expit(t)
    general = MR.total_variance(p, p * (1.0 - p))
    assert np.allclose(var, general, rtol=1e-12, atol=1e-15)
    assert np.array_equal(mean, p.mean(axis=0))
    for family in ("linear", "poisson"):                # the other two ARE that expression
        X, _, W, b = MR.LR.inputs(family, 37, 50, 9, True)
        t = MR.LR.linear_predictor(X, W, b)
        mu, v, _, _ = MR.conditional_moments(family, t, 0.5)
        mean, var = MR.moments_of_t(family, t, 0.5)
        assert np.array_equal(var, MR.total_variance(mu, v)) and np.array_equal(mean, mu.mean(axis=0))


def test_comparator_single_draw_has_the_conditional_variance():
    from tests import moments_ref as MR
    for family in MR.FAMILIES:
        X, _, W, b = MR.LR.inputs(family, 1, 40, 7, True)
        t = MR.LR.linear_predictor(X, W, b)
        mu, v, _, _ = MR.conditional_moments(family, t, MR.SIGMA[family])
        mean, var = MR.moments_of_t(family, t, MR.SIGMA[family])
        assert np.array_equal(mean, mu[0])
        if family == "logistic":
            assert np.allclose(var, v[0], rtol=1e-15, atol=0)
        else:
            assert np.array_equal(var, v[0])
    sig = MR.SIGMA["linear"]
    assert np.all(MR.moments_of_t("linear", np.full((9, 4), 1.25), sig)[1] == sig ** 2)      # equal draws: no between-draw term
    m, v = MR.moments_of_t("poisson", np.full((9, 4), 1.25), 1.0)
    assert np.array_equal(m, v)


def test_comparator_non_finite_rule():
    from tests import moments_ref as MR
    t = np.array([[1.0, 95.0, 2.0, 200.0, np.nan], [0.5, 1.0, 3.0, 150.0, 95.0]])
    m, v = MR.moments_of_t("poisson", t, 1.0)
    assert np.isfinite(m[[0, 2]]).all() and np.isfinite(v[[0, 2]]).all()
    assert np.isposinf(m[[1, 3]]).all() and np.isposinf(v[[1, 3]]).all()      # one draw overflows, every draw overflows: never NaN
    assert np.isnan(m[4]) and np.isnan(v[4])                                  # NaN before inf
    for family in MR.FAMILIES:
        m, v = MR.moments_of_t(family, np.array([[0.3, np.nan], [0.1, 0.2]]), 0.5)
        assert np.isfinite(m[0]) and np.isfinite(v[0]) and np.isnan(m[1]) and np.isnan(v[1])
    # a finite float64 variance beyond float32's range is +inf beside a finite mean
    m, v = MR.moments_of_t("poisson", np.log(np.array([[1e30], [3e30]])), 1.0)
    assert np.isfinite(m[0]) and np.isposinf(v[0])
    ok = np.array([1.0, np.inf, np.nan, -np.inf])
    MR.assert_close(ok, ok, np.array([1e-6, 0, 0, 0]), "classes")
    for bad, msg in ((np.array([1.0, np.nan, np.nan, -np.inf]), r"\+inf entries differ|NaN entries differ"),
                     (np.array([1.0, np.inf, 0.0, -np.inf]), "NaN entries differ"),
                     (np.array([1.0, np.inf, np.nan, np.inf]), "inf entries differ"),
                     (np.array([1.0 + 3e-6, np.inf, np.nan, -np.inf]), "above the bound")):
        with pytest.raises(AssertionError, match=msg):
            MR.assert_close(bad, ok, np.array([1e-6, 0, 0, 0]), "classes")


def test_cancellation_problem_tells_a_float32_sum_of_squares_from_the_bound():
    """The bound of the cancellation case is far below what a float32 sum of mu^2 loses, so the GPU test discriminates."""
    from tests import moments_ref as MR
    X, W, b = MR.cancellation_problem()
    sig = MR.SIGMA["linear"]
    t = MR.LR.linear_predictor(X, W, b)
    assert np.abs(t - 1e4).max() < 10.0 and 0.5e-2 < t.std(axis=0).min() and t.std(axis=0).max() < 2e-2
    _, var = MR.moments64("linear", X, W, b, sig)
    _, b_var = MR.bounds("linear", X, W, b, sig)
    assert np.all(b_var < 1e-3)
    bad = MR.float32_sum_of_squares_variance(t, sig)
    # its result moves in steps of 8 / n around sigma^2: a row may land on the step next to the truth by chance, most are far off
    assert np.mean(np.abs(bad - var) > 100 * b_var) > 0.9
    # the float32-rounded mu themselves, accumulated in float64, pass
    mu32 = t.astype(np.float32).astype(np.float64)
    good = sig ** 2 + ((mu32 - mu32.mean(axis=0)) ** 2).mean(axis=0)
    assert np.all(np.abs(good - var) <= b_var)


def test_sweep_adds_the_draw_counts_around_one_wave():
    from tests import moments_ref as MR
    cases = MR.sweep_cases()
    assert set(MR.LR.sweep_cases()) <= set(cases)
    for family in MR.FAMILIES:
        mine = [c for c in cases if c[0] == family]
        assert {64, 65} <= {c[1] for c in mine}
        assert sum(1 for c in mine if c[1:4] == MR.CORNER) == 1
        for n in (64, 65):
            assert {c[4] for c in mine if c[1] == n} == {False, True}


def test_link_tolerance_is_four_times_the_comparators_float32_error():
    """LINK_RTOL is built on the float32 error of torch's own links at the sweep's float32 linear predictors; recomputed here on the
    CPU: no figure may have grown past the one tests/moments_ref.py records."""
    from tests import moments_ref as MR
    for family in MR.FAMILIES:
        r, where = MR.float32_link_calibration(family)
        print(f"{family}: float32 torch against float64 at the same float32 t: {r:.3e} at (n, rows, d, intercept) = {where}")
        assert 0 <= r <= MR.LINK_MEASURED[family], (family, r)
        assert (r > 0) == (family != "linear")
        assert MR.LINK_RTOL[family] == 4 * MR.LINK_MEASURED[family]
