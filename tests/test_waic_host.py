"""d3p_amd.criteria (WAIC and pairwise comparison), host side: the calibration of tests/waic_ref.py's bound of p_waic, the module
surface and the C entries' declarations, waic's refusals before a device is touched, and compare on hand-made CPU results."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import loglik_ref as LR
from tests import mixture_density_ref as MR
from tests import waic_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("criteria reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


# ------------------------------------------------------------------------------------------------ calibration
def test_float32_restatement_stays_inside_the_bound_regression():
    """ll with float32's error in it (float32 product, float32 link) fed to a float64 variance: inside bound_v on every sweep
    case with n >= 2 at both ddof.  Recorded while the bound was written: largest error / bound 0.0097."""
    worst, where = 0.0, None
    for family, n, rows, d, intercept in LR.sweep_cases():
        if n < 2:
            continue
        X, y, W, b = LR.inputs(family, n, rows, d, intercept)
        ll32 = WR.regression_ll32(family, X, y, W, b)
        for ddof in (0, 1):
            ref = WR.regression_reference(family, n, rows, d, intercept, ddof)
            err = np.abs(WR.pwaic64(ll32, ddof) - ref["v"])
            assert np.all(err <= ref["bound_v"]), (family, n, rows, d, intercept, ddof)
            ratio = float(np.max(err / ref["bound_v"]))
            if ratio > worst:
                worst, where = ratio, (family, n, rows, d, intercept, ddof)
            # the bound says something: it is a small part of the variance
            assert np.all(ref["bound_v"] <= 0.05 * ref["v"]), (family, n, rows, d, intercept, ddof)
    print(f"regression: largest error / bound {worst:.4f} at {where}")
    assert 0.0 < worst <= 1.0


def test_float32_restatement_stays_inside_the_bound_mixture():
    """The same with MR.a32_restated and MR.ll32_restated.  Recorded: largest error / bound 0.049."""
    worst, where = 0.0, None
    for kind in MR.KINDS:
        for case in WR.MIXTURE_CASES:
            ll32 = None
            for ddof in (0, 1):
                ref = WR.mixture_reference(kind, *case, ddof)
                ll32 = WR.mixture_ll32(ref) if ll32 is None else ll32
                err = np.abs(WR.pwaic64(ll32, ddof) - ref["v"])
                assert np.all(err <= ref["bound_v"]), (kind, case, ddof)
                ratio = float(np.max(err / ref["bound_v"]))
                if ratio > worst:
                    worst, where = ratio, (kind, case, ddof)
    print(f"mixture: largest error / bound {worst:.4f} at {where}")
    assert 0.0 < worst <= 1.0


def test_reference_variance_and_its_special_rows():
    ll = np.array([[1.0, 2.0, -np.inf], [3.0, 2.0, -np.inf], [5.0, 2.0, 0.0]])
    assert np.array_equal(WR.pwaic64(ll, 1), [4.0, 0.0, np.inf]) and np.array_equal(WR.pwaic64(ll, 0), [8.0 / 3.0, 0.0, np.inf])
    b = WR.bound_v(ll, np.array([0.5, 0.5, 0.5]), 1)
    assert b[0] == (4 * 0.5 * 4.0 + 4 * 3 * 0.25) / 2 + WR.ROUNDING * 4.0 and b[1] == (4 * 3 * 0.25) / 2 and b[2] == 0.0
    # the bound holds for any perturbation of at most beta per element
    r = np.random.default_rng(3)
    x = r.normal(size=(9, 50))
    for _ in range(20):
        beta = 10.0 ** r.uniform(-6, 0, 50)
        moved = x + beta * r.uniform(-1.0, 1.0, x.shape)
        for ddof in (0, 1):
            assert np.all(np.abs(WR.pwaic64(moved, ddof) - WR.pwaic64(x, ddof)) <= WR.bound_v(x, beta, ddof))


def test_overflow_constructions_are_where_the_gpu_tests_mean_them():
    n, rows, d, X, y, W, t = WR.overflow_problem(False)
    over = t > 89.0
    assert over[2].sum() == 9 and not over[[0, 1, 3, 4]].any()
    ll = LR.ll64("poisson", X, y, W, None, 1.0)
    assert np.array_equal(np.isneginf(ll), over) and np.isfinite(LR.lppd64(ll)).all()
    assert np.array_equal(np.isinf(WR.pwaic64(ll, 1)), over[2])
    n, rows, d, X, y, W, t = WR.overflow_problem(True)
    dead = (t > 89.0).all(axis=0)
    assert dead[:10].all() and not dead[10:].any()


# ------------------------------------------------------------------------------------------------ surface
def test_module_surface_and_entry_points():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import criteria as CR
    assert d3p_amd.criteria is CR and "criteria" in d3p_amd.__all__
    assert CR.__all__ == ["waic", "posterior_waic", "compare", "WAICResult", "ComparisonResult"]
    assert CR.WAICResult._fields == ("elpd_waic", "p_waic", "waic", "se", "n_draws", "n_rows", "pointwise")
    assert CR.ComparisonResult._fields == ("elpd_diff", "se_diff")
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        hdr = f.read()
    for name in ("d3p_loglik_waic", "d3p_gmm_loglik_waic"):
        assert re.search(r"\bint " + name + r"\(", hdr) and name in L.SIGNATURES, name
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    lib = L.load()
    assert lib.d3p_abi_version() == 9 and hasattr(lib, "d3p_loglik_waic") and hasattr(lib, "d3p_gmm_loglik_waic")
    assert len(L.SIGNATURES["d3p_loglik_waic"][1]) == 13 and len(L.SIGNATURES["d3p_gmm_loglik_waic"][1]) == 11
    csrc = os.path.join(ROOT, "d3p_amd", "csrc")
    defs = 0
    for name in os.listdir(csrc):
        with open(os.path.join(csrc, name)) as f:
            defs += len(re.findall(r"float loglik_value\(", f.read()))
    assert defs == 1                                                     # one definition of the likelihood


def test_import_stays_lazy():
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.criteria' not in sys.modules; " \
           "d3p_amd.criteria; assert 'd3p_amd.criteria' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------------------------------------ refusals
def test_waic_refuses_before_the_device(no_device):
    from d3p_amd import criteria as CR
    from d3p_amd.models import (AutoDiagonalNormal, GaussianMean, GaussianMixtureGuide, GaussianMixtureModel, LinearRegression,
                                LogisticRegression, PoissonRegression, VAEModel)
    X, y = np.zeros((6, 3), np.float32), np.zeros(6, np.float32)
    good = {"w": np.zeros((4, 3), np.float32)}
    for bad_model in (GaussianMean(3), VAEModel(2, 4)):
        with pytest.raises(TypeError):
            CR.waic(bad_model, good, X, y)
        with pytest.raises(TypeError):
            CR.posterior_waic(torch.zeros(2, dtype=torch.int32), 4, bad_model, (X, y), None, {})
    gm = GaussianMixtureModel()
    mix = {"pis": np.full((4, 3), 1 / 3, np.float32), "mus": np.zeros((4, 3, 2), np.float32), "sigs": np.ones((4, 3, 2), np.float32)}
    obs = np.zeros((10, 2), np.float32)
    for model in (LogisticRegression(3), LinearRegression(3), PoissonRegression(3)):
        with pytest.raises(ValueError, match="ddof"):
            CR.waic(model, {"w": np.zeros((1, 3), np.float32)}, X, y)                  # n = 1 at ddof = 1
        with pytest.raises(ValueError, match="ddof"):
            CR.waic(model, {"w": np.zeros(3, np.float32)}, X, y, ddof=1)               # a single sample
        for ddof in (2, -1, 0.5, None, True):
            with pytest.raises(ValueError, match="ddof"):
                CR.waic(model, good, X, y, ddof=ddof)
        with pytest.raises(ValueError, match="y is missing"):
            CR.waic(model, good, X)
        with pytest.raises(ValueError):
            CR.waic(model, good)
        with pytest.raises(ValueError):
            CR.waic(model, {"intercept": np.zeros(4)}, X, y)
        guide = AutoDiagonalNormal(model)
        key = torch.zeros(2, dtype=torch.int32)                                        # (a CPU tensor: the key check is the last)
        params = {"auto_loc": np.zeros(3, np.float32), "auto_scale": np.ones(3, np.float32)}
        with pytest.raises(ValueError, match="ddof"):
            CR.posterior_waic(key, 1, model, (X, y), guide, params)
        with pytest.raises(ValueError, match="ddof"):
            CR.posterior_waic(key, 4, model, (X, y), guide, params, ddof=2)
        with pytest.raises(ValueError, match="y is missing"):
            CR.posterior_waic(key, 4, model, (X,), guide, params)
        with pytest.raises(TypeError):
            CR.posterior_waic(key, 4, model, (X, y), guide, params)                    # every host check passed: the key is refused
    with pytest.raises(ValueError, match="ddof"):
        CR.waic(gm, {name: v[:1] for name, v in mix.items()}, obs)                     # n = 1 at ddof = 1
    with pytest.raises(ValueError, match="ddof"):
        CR.waic(gm, mix, obs, ddof=2)
    with pytest.raises(ValueError, match="obs is required"):
        CR.waic(gm, mix)
    with pytest.raises(ValueError):
        CR.waic(gm, {"pis": mix["pis"]}, obs)
    gg = GaussianMixtureGuide(gm)
    gparams = {"alpha_log": np.zeros(3, np.float32), "mus_loc": np.zeros((3, 2), np.float32)}
    key = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="ddof"):
        CR.posterior_waic(key, 1, gm, (3, obs, 10, 2), gg, gparams)
    with pytest.raises(ValueError, match="ddof"):
        CR.posterior_waic(key, 4, gm, (3, obs, 10, 2), gg, gparams, ddof=3)
    with pytest.raises(ValueError, match="obs is required"):
        CR.posterior_waic(key, 4, gm, (3, None, 10, 2), gg, gparams)
    with pytest.raises(TypeError):
        CR.posterior_waic(key, 4, gm, (3, obs, 10, 2), gg, gparams)


# ------------------------------------------------------------------------------------------------ compare
def _hand_made(elpd, n=7):
    from d3p_amd import criteria as CR
    e = torch.tensor(np.asarray(elpd, np.float32))
    pw = torch.zeros_like(e)
    return CR._result(e + pw, pw, n, True)


def test_compare_against_numpy_on_cpu_results():
    from d3p_amd import criteria as CR
    r = np.random.default_rng(11)
    rows = 301
    ea = (-1.0 + 0.3 * r.normal(size=rows)).astype(np.float32)
    eb = (ea + 0.05 + 0.2 * r.normal(size=rows)).astype(np.float32)
    a, b = _hand_made(ea), _hand_made(eb, n=9)
    assert a.n_rows == rows and a.n_draws == 7 and a.pointwise["elpd_waic"].device.type == "cpu"
    WR.check_totals(a, "hand-made a")
    got = CR.compare(a, b)
    assert isinstance(got, CR.ComparisonResult) and got.elpd_diff.dtype == got.se_diff.dtype == torch.float64 and got.elpd_diff.dim() == 0
    diff = ea.astype(np.float64) - eb.astype(np.float64)
    terms = rows * (diff - diff.mean()) ** 2 / (rows - 1)
    assert abs(float(got.elpd_diff) - diff.sum()) <= WR.sum_bound(diff)
    assert abs(float(got.se_diff) ** 2 - terms.sum()) <= WR.sum_bound(terms) + 2.0 ** -51 * terms.sum()
    back = CR.compare(b, a)
    assert float(back.elpd_diff) == -float(got.elpd_diff) and float(back.se_diff) == float(got.se_diff)
    same = CR.compare(a, a)
    assert float(same.elpd_diff) == 0.0 and float(same.se_diff) == 0.0
    one = CR.compare(_hand_made([-1.0]), _hand_made([-2.0]))
    assert float(one.elpd_diff) == 1.0 and np.isnan(float(one.se_diff))


def test_compare_refuses_results_without_rows_in_common():
    from d3p_amd import criteria as CR
    a = _hand_made([-1.0, -2.0, -3.0])
    with pytest.raises(ValueError, match="pointwise"):
        CR.compare(a, a._replace(pointwise=None))
    with pytest.raises(ValueError, match="pointwise"):
        CR.compare((1.0, 2.0), a)
    with pytest.raises(ValueError, match="rows"):
        CR.compare(a, _hand_made([-1.0, -2.0]))
