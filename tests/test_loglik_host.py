"""d3p_amd.infer_util (log_likelihood, log predictive densities), host side: the module and its C entry points exist, every
validation error is raised before a device is touched, the unsupported models are refused -- and the self-checks of
tests/loglik_ref.py, the comparator every test of tests/test_gpu_loglik.py rests on."""
import math
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
        raise AssertionError("infer_util reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


def test_module_imports_and_is_exported():
    import d3p_amd
    from d3p_amd import infer_util as U
    assert d3p_amd.infer_util is U
    assert U.__all__ == ["log_likelihood", "log_predictive_density", "posterior_log_predictive_density"]
    for name in U.__all__:
        assert "UNSCALED" in getattr(U, name).__doc__, name


def test_header_and_binding_declare_both_entry_points():
    import d3p_amd._lib as L
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define D3P_ABI_VERSION 9\b", header)
    for name in ("d3p_loglik_rows", "d3p_loglik_lppd"):
        assert re.search(r"\bint %s\(void\* stream, const d3p_logreg_model\* model," % name, header), name
        res, args = L.SIGNATURES[name]
        assert res is L.C.c_int and len(args) == 11
    assert os.path.join(os.path.dirname(L.__file__), "csrc", "d3p_loglik.hip") in L._SRC


def test_library_exports_the_entry_points():
    import d3p_amd._lib as L
    lib = L.load()
    assert lib.d3p_abi_version() == 9
    assert lib.d3p_loglik_rows.argtypes == L.SIGNATURES["d3p_loglik_rows"][1] and lib.d3p_loglik_lppd.restype is L.C.c_int


@pytest.mark.parametrize("fn", ["log_likelihood", "log_predictive_density"])
def test_validation_comes_before_the_device(no_device, fn):
    from d3p_amd import infer_util as U
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    f = getattr(U, fn)
    X, y = torch.zeros(5, 3), torch.zeros(5)
    w, b = torch.zeros(4, 3), torch.zeros(4)
    plain, icpt = LogisticRegression(3), LinearRegression(3, intercept=True)
    with pytest.raises(ValueError, match="'w' is missing"):
        f(plain, {}, X, y)
    with pytest.raises(ValueError, match="'w' is missing"):
        f(plain, None, X, y)
    with pytest.raises(ValueError, match=r"posterior_samples\['w'\]"):
        f(plain, {"w": torch.zeros(4, 2)}, X, y)
    with pytest.raises(ValueError, match=r"posterior_samples\['w'\]"):
        f(plain, {"w": np.zeros((2, 4, 3), np.float32)}, X, y)
    with pytest.raises(ValueError, match="'intercept' is missing"):
        f(icpt, {"w": w}, X, y)
    with pytest.raises(ValueError, match=r"posterior_samples\['intercept'\]"):
        f(icpt, {"w": w, "intercept": torch.zeros(3)}, X, y)
    with pytest.raises(ValueError, match="y is missing"):
        f(plain, {"w": w}, X)
    with pytest.raises(ValueError, match="y is missing"):
        f(plain, {"w": w}, X, None, 5)
    with pytest.raises(ValueError, match="5 labels expected"):
        f(plain, {"w": w}, X, torch.zeros(4))
    with pytest.raises(ValueError, match="2-D"):
        f(plain, {"w": w}, torch.zeros(5), y)
    with pytest.raises(ValueError, match="2-D"):
        f(plain, {"w": w}, torch.zeros(5, 3, 1), y)
    with pytest.raises(ValueError, match="model_args"):
        f(plain, {"w": w})
    with pytest.raises(ValueError, match="columns"):
        f(LogisticRegression(4), {"w": w}, X, y)
    with pytest.raises(ValueError, match="labels must be integers"):
        f(PoissonRegression(3, validate_args=True), {"w": w}, X, torch.tensor([0.0, 1.0, 2.5, 0.0, 1.0]))
    with pytest.raises(ValueError, match="labels must be integers"):
        f(PoissonRegression(3, validate_args=True), {"w": w}, X, torch.tensor([0.0, 1.0, -1.0, 0.0, 1.0]))
    # ... and what passes every check goes on to the device
    for model, samples in ((plain, {"w": w}), (icpt, {"w": w, "intercept": b.reshape(4, 1)}), (plain, {"w": np.zeros(3, np.float32)}),
                           (PoissonRegression(3), {"w": w}), (PoissonRegression(3, validate_args=True), {"w": w})):
        with pytest.raises(AssertionError, match="reached require_device"):
            f(model, samples, X, y, 5)


def test_posterior_density_validates_before_the_device(no_device):
    from d3p_amd import infer_util as U
    from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, LinearRegression, LogisticRegression, MeanFieldGuide,
                                PoissonRegression, VAEGuide, VAEModel)
    f = U.posterior_log_predictive_density
    X, y = torch.zeros(5, 3), torch.zeros(5)
    lin, logi = LinearRegression(3, intercept=True), LogisticRegression(3, intercept=True)
    auto = {"auto_loc": torch.zeros(4), "auto_scale": torch.ones(4)}
    with pytest.raises(ValueError, match="'auto_scale' is missing"):
        f(None, 4, lin, (X, y), AutoDiagonalNormal(lin), {"auto_loc": torch.zeros(4)})
    with pytest.raises(ValueError, match="4 values expected"):
        f(None, 4, lin, (X, y), AutoDiagonalNormal(lin), {"auto_loc": torch.zeros(3), "auto_scale": torch.ones(4)})
    with pytest.raises(ValueError, match="params"):
        f(None, 4, lin, (X, y), AutoDiagonalNormal(lin), None)
    with pytest.raises(ValueError, match="'w_std_log' is missing"):
        f(None, 4, lin, (X, y), DiagonalNormalGuide(lin), {"w_loc": torch.zeros(4)})
    with pytest.raises(ValueError, match="n must be >= 1"):
        f(None, 0, lin, (X, y), AutoDiagonalNormal(lin), auto)
    with pytest.raises(ValueError, match="y is missing"):
        f(None, 4, lin, (X,), AutoDiagonalNormal(lin), auto)
    with pytest.raises(ValueError, match="5 labels expected"):
        f(None, 4, lin, (X, torch.zeros(6)), AutoDiagonalNormal(lin), auto)
    with pytest.raises(ValueError, match="2-D"):
        f(None, 4, lin, (torch.zeros(5), y), AutoDiagonalNormal(lin), auto)
    with pytest.raises(ValueError, match="labels must be integers"):
        pm = PoissonRegression(3, intercept=True, validate_args=True)
        f(None, 4, pm, (X, torch.full((5,), 0.5)), AutoDiagonalNormal(pm), auto)
    # the two-site guide is built for logistic regression only; a guide of another family is refused
    for model in (lin, PoissonRegression(3, intercept=True)):
        with pytest.raises(TypeError, match="MeanFieldGuide is not supported"):
            f(None, 4, model, (X, y), MeanFieldGuide(model), {})
    with pytest.raises(TypeError, match="VAEGuide is not supported"):
        f(None, 4, logi, (X, y), VAEGuide(VAEModel(2, 3)), {})
    with pytest.raises(ValueError, match="'w_loc' is missing"):
        f(None, 4, logi, (X, y), MeanFieldGuide(logi), {})
    with pytest.raises(TypeError, match="rng_key"):          # (the key is the last of the checks, still before the device)
        f(None, 4, lin, (X, y), AutoDiagonalNormal(lin), auto)


def test_unsupported_models_raise_type_error(no_device):
    from d3p_amd import infer_util as U
    from d3p_amd.models import AutoDiagonalNormal, GaussianMean, GaussianMixtureModel, VAEModel
    X, y = torch.zeros(5, 3), torch.zeros(5)
    for model in (GaussianMean(3), GaussianMixtureModel(2, 3), VAEModel(2, 4)):
        for call in (lambda: U.log_likelihood(model, {"w": torch.zeros(2, 3)}, X, y),
                     lambda: U.log_predictive_density(model, {"w": torch.zeros(2, 3)}, X, y),
                     lambda: U.posterior_log_predictive_density(None, 2, model, (X, y), AutoDiagonalNormal(model), {})):
            with pytest.raises(TypeError, match="log_likelihood: unsupported model " + type(model).__name__):
                call()


def test_packed_samples_are_read_in_place(monkeypatch):
    """The (n, D) buffer of the kernels is a VIEW when `w` and `intercept` already are columns of one buffer, whichever comes first."""
    from d3p_amd import infer_util as U
    buf = torch.arange(40, dtype=torch.float32).reshape(5, 8)
    monkeypatch.setattr(U.M, "_device", lambda: buf.device)      # (the rule is about layout; the real one asks for the current GPU)
    first, ld, w_off, b_col = U._packed_view(buf[:, 1:4], buf[:, 4], 5, 3)
    assert (first.data_ptr(), ld, w_off, b_col) == (buf[:, 1:].data_ptr(), 8, 0, 3)
    first, ld, w_off, b_col = U._packed_view(buf[:, 2:5], buf[:, 0], 5, 3)
    assert (first.data_ptr(), ld, w_off, b_col) == (buf.data_ptr(), 8, 2, 0)
    first, ld, w_off, b_col = U._packed_view(buf[:, :3], None, 5, 3)
    assert (first.data_ptr(), ld, w_off, b_col) == (buf.data_ptr(), 8, 0, -1)
    first, ld, w_off, b_col = U._packed_view(buf[2:3, :3], buf[2:3, 3], 1, 3)
    assert (first.data_ptr(), w_off, b_col) == (buf[2:].data_ptr(), 0, 3) and ld >= 4
    assert U._packed_view(buf[:, 1:4], buf[:, 2], 5, 3) is None                     # the intercept inside the weights
    assert U._packed_view(buf[:, 1:4], torch.zeros(5), 5, 3) is None                # two buffers
    assert U._packed_view(buf[:, ::2][:, :3], buf[:, 7], 5, 3) is None              # strided weights
    assert U._packed_view(buf[:, 1:4], buf[:, 4].repeat(2)[::2], 5, 3) is None      # an intercept with another row stride
    assert U._packed_view(buf.double()[:, 1:4], None, 5, 3) is None                 # not float32
    assert U._packed_view(buf[:, :1].expand(5, 3), None, 5, 3) is None              # overlapping rows (stride 0 along the weights)


# ---------------------------------------------------------------- the comparator
def test_comparator_logistic_is_minus_softplus_by_hand():
    from tests import loglik_ref as LR
    t = np.array([[-30.0, -4.0, -0.3, 0.0, 0.7, 4.0, 30.0]])
    sp = lambda x: max(x, 0.0) + math.log1p(math.exp(-abs(x)))      # noqa: E731
    one = LR.ll_of_t("logistic", t, np.ones(7), 1.0)
    zero = LR.ll_of_t("logistic", t, np.zeros(7), 1.0)
    for j, v in enumerate(t[0]):
        assert abs(one[0, j] - (-sp(-v))) <= 1e-13 * max(1.0, abs(sp(-v)))
        assert abs(zero[0, j] - (-sp(v))) <= 1e-13 * max(1.0, abs(sp(v)))


def test_comparator_is_the_product_then_glm_refs_likelihood():
    from tests import glm_ref as R
    from tests import loglik_ref as LR
    for family in LR.FAMILIES:
        X, y, W, b = LR.inputs(family, 3, 5, 4, True)
        ll = LR.ll64(family, X, y, W, b, LR.SIGMA[family])
        assert ll.shape == (3, 5)
        for s in range(3):
            t = X.astype(np.float64) @ W[s].astype(np.float64) + float(b[s])
            assert np.abs(t).max() <= 4.0
            exp = R._loglik(family, torch.tensor(t), torch.tensor(y, dtype=torch.float64), LR.SIGMA[family]).numpy()
            assert np.array_equal(ll[s], exp)
        lp = LR.lppd64(ll)
        assert np.allclose(lp, np.log(np.exp(ll).mean(axis=0)), rtol=1e-12, atol=0)


def test_comparator_poisson_overflow_and_all_minus_inf_rows():
    """float32's range: exp(t) beyond 3.4e38 is -inf in the comparator, finite below; a log-sum-exp over -inf only is -inf, not NaN."""
    from tests import loglik_ref as LR
    t = np.array([[88.0, 89.5, 2.0], [1.0, 95.0, 0.5]])
    ll = LR.ll_of_t("poisson", t, np.array([3.0, 0.0, 1.0]), 1.0)
    assert np.array_equal(np.isneginf(ll), [[False, True, False], [False, True, False]]) and not np.isnan(ll).any()
    lp = LR.lppd64(ll)
    assert np.isfinite(lp[0]) and np.isneginf(lp[1]) and np.isfinite(lp[2])
    assert abs(lp[0] - (ll[1, 0] - math.log(2) + math.log1p(math.exp(ll[0, 0] - ll[1, 0])))) < 1e-12
    allinf = LR.logsumexp_rows(np.full((4, 3), -np.inf))
    assert np.array_equal(np.isneginf(allinf), [True] * 3)
    with pytest.raises(AssertionError, match="NaN"):
        LR.assert_close(np.array([np.nan]), np.array([0.0]), np.array([1.0]), "nan")
    with pytest.raises(AssertionError, match="-inf entries differ"):
        LR.assert_close(np.array([-1e30]), np.array([-np.inf]), np.array([1.0]), "inf")
    with pytest.raises(AssertionError, match="above the bound"):
        LR.assert_close(np.array([1.0 + 3e-6]), np.array([1.0]), np.array([2e-6]), "far")
    LR.assert_close(np.array([-np.inf, 1.0 + 1e-6]), np.array([-np.inf, 1.0]), np.array([0.0, 2e-6]), "ok")


def test_sweep_covers_every_tile_edge_with_two_partners():
    from tests import loglik_ref as LR
    shapes = LR.SHAPES + [LR.CORNER]
    assert LR.SHAPES.count(LR.CORNER) == 0
    axes = ({1, 31, 128, 129, 257}, {1, 63, 128, 129, 300}, {1, 31, 32, 33, 513})
    for ax, values in enumerate(axes):
        assert {s[ax] for s in shapes} == values
        for v in values:
            for other in set(range(3)) - {ax}:
                assert len({s[other] for s in shapes if s[ax] == v}) >= 2, (ax, v, other)
    cases = LR.sweep_cases()
    for family in LR.FAMILIES:
        assert sum(1 for c in cases if c[0] == family and c[1:4] == LR.CORNER) == 1
        assert {c[4] for c in cases if c[0] == family} == {False, True}


def test_link_tolerance_is_four_times_the_comparators_float32_error():
    """LINK_RTOL is built on the float32 error of torch's own likelihoods at the sweep's float32 linear predictors; recomputed here on
    the CPU: no figure may have grown past the one tests/loglik_ref.py records."""
    from tests import loglik_ref as LR
    for family in LR.FAMILIES:
        r, where = LR.float32_link_calibration(family)
        print(f"{family}: float32 torch against float64 at the same float32 t: {r:.3e} at (n, rows, d, intercept) = {where}")
        assert 0 < r <= LR.LINK_MEASURED[family], (family, r)
        assert LR.LINK_RTOL[family] == 4 * LR.LINK_MEASURED[family]
