"""Host checks of the clipping diagnostics (d3p_amd/clipping.py): the comparator tests/clipping_ref.py against hand-computed cases, the
positions over the finite count, suggest_clipping_threshold, the refusals that need no device, and the calibration of the bound the
GPU tests use."""
import math

import numpy as np
import pytest
import torch

from tests import clipping_ref as CR
from tests import glm_ref as R


# ---------------------------------------------------------------- the reference against hand-computed cases
def test_profile_ref_by_hand():
    v = np.array([3.0, 0.0, 1.0, np.inf, 2.0, np.nan, 4.0], np.float32)       # finite: 0 1 2 3 4
    p = CR.profile_ref(v, (2.0, 8.0), (0.0, 0.5, 0.625, 1.0))
    assert (p["n"], p["n_finite"], p["n_nonfinite"]) == (7, 5, 2)
    assert p["mean"] == 2.0 and p["mean_sq"] == 6.0 and p["rms"] == math.sqrt(6.0) and p["max"] == 4.0
    assert p["quantiles"] == (0.0, 2.0, 2.5, 4.0)                             # h = 4 p: 0, 2, 2.5, 4
    assert p["n_clipped"] == (4, 2)                                           # 3, 4 and the two non-finite | the two non-finite (strict >)
    assert p["clipped_fraction"] == (4 / 7, 2 / 7)
    # min(1, C / norm): 2/3, 1 (zero norm), 1, 0, 1 (equal to C: not clipped), 0, 2/4
    assert p["mean_clip_factor"][0] == pytest.approx((2 / 3 + 1 + 1 + 0 + 1 + 0 + 0.5) / 7, rel=1e-15)
    assert p["mean_clip_factor"][1] == pytest.approx(5 / 7, rel=1e-15)


def test_profile_ref_without_finite_values():
    p = CR.profile_ref(np.array([np.inf, np.nan], np.float32), (1.0,), (0.5,))
    assert p["n_finite"] == 0 and p["n_clipped"] == (2,) and p["mean_clip_factor"] == (0.0,)
    assert all(math.isnan(x) for x in (p["mean"], p["rms"], p["max"], p["quantiles"][0]))


def test_norms_ref_by_hand():
    """Linear regression, d = 1, no intercept, eps = 0, exp guide with unc = 0 (s = 1): z = loc, t = x loc,
    d/dloc = (N (t - y) x / sigma^2 + z / prior^2) / obs, d/dunc = (d/dz) s eps - 1 / obs = -1 / obs."""
    h = R.hyper(1, False, prior_w=2.0, lik_scale=10.0, obs_scale=5.0, sigma=0.5)
    X, y = np.array([[3.0]], np.float32), np.array([1.0], np.float32)
    loc, unc, eps = np.array([0.5], np.float32), np.array([0.0], np.float32), np.zeros((1, 1), np.float32)
    norms, L = CR.norms_ref("linear", h, loc, unc, X, y, eps, "exp")
    g_loc = (10.0 * (1.5 - 1.0) * 3.0 / 0.25 + 0.5 / 4.0) / 5.0
    assert norms[0] == pytest.approx(math.hypot(g_loc, -1.0 / 5.0), rel=1e-14)


# ---------------------------------------------------------------- positions over the finite count
def test_positions_are_taken_over_the_finite_count():
    from d3p_amd.intervals import positions
    for n in (1, 2, 5, 257, 1000003):
        assert positions(CR.PROFILE_PROBS, n) == CR.positions(CR.PROFILE_PROBS, n)
    assert CR.positions((0.0, 0.5, 0.625, 1.0), 5) == [(0, 0.0), (2, 0.0), (2, 0.5), (4, 0.0)]
    v = np.array([3.0, np.inf, 1.0, np.nan, 2.0], np.float32)                 # n = 5, n_finite = 3: the median is the 2nd finite value
    (lo, g), = CR.positions((0.5,), 3)
    assert (lo, g) == (1, 0.0) and CR.profile_ref(v, (), (0.5,))["quantiles"] == (2.0,)


# ---------------------------------------------------------------- suggest_clipping_threshold
def _profile(**kw):
    from d3p_amd.clipping import ClippingProfile
    base = dict(n=10, n_nonfinite=0, mean=1.0, rms=1.2, max=3.0, probs=(0.5, 0.9), quantiles=(0.8, 2.5), thresholds=(1.0,),
                clipped_fraction=(0.4,), mean_clip_factor=(0.9,))
    base.update(kw)
    return ClippingProfile(**base)


def test_suggest_clipping_threshold():
    from d3p_amd.clipping import suggest_clipping_threshold
    assert suggest_clipping_threshold(_profile()) == 0.8
    assert suggest_clipping_threshold(_profile(), prob=0.9) == 2.5
    with pytest.raises(ValueError, match="not among"):
        suggest_clipping_threshold(_profile(), prob=0.75)
    with pytest.raises(ValueError, match="finite and > 0"):
        suggest_clipping_threshold(_profile(quantiles=(float("nan"), 2.5)))
    with pytest.raises(ValueError, match="finite and > 0"):
        suggest_clipping_threshold(_profile(quantiles=(0.0, 2.5)))
    with pytest.raises(TypeError):
        suggest_clipping_threshold({"probs": (0.5,), "quantiles": (1.0,)})


# ---------------------------------------------------------------- refusals that need no device
def _svi(model, guide=None, K=1, **kw):
    from d3p_amd.models import Adam, AutoDiagonalNormal, Trace_ELBO
    from d3p_amd.svi import DPSVI
    return DPSVI(model, guide or AutoDiagonalNormal(model), Adam(1e-3), Trace_ELBO(num_particles=K), 1.0, 1.0, **kw)


def _no_device(monkeypatch):
    import d3p_amd._lib as L

    def boom(*a, **k):
        raise AssertionError("a device call was made before the refusal")
    monkeypatch.setattr(L, "require_device", boom)
    monkeypatch.setattr(L, "load", boom)


def test_refusals_before_any_device_call(monkeypatch):
    import d3p_amd._lib as L
    from d3p_amd import clipping as CL
    from d3p_amd.models import (GaussianMean, GaussianMixtureGuide, GaussianMixtureModel, LogisticRegression, PoissonRegression, VAEGuide,
                                VAEModel)
    _no_device(monkeypatch)
    X, y = np.zeros((5, 4), np.float32), np.zeros(5, np.float32)
    with pytest.raises(TypeError, match="GaussianMean"):
        CL.gradient_norms(_svi(GaussianMean(4)), None, X, y)
    gmm = GaussianMixtureModel(k=2)
    with pytest.raises(TypeError, match="GaussianMixtureModel"):
        CL.gradient_norms(_svi(gmm, GaussianMixtureGuide(gmm)), None, X, y)
    vae = VAEModel(hidden_dim=8, z_dim=2)
    with pytest.raises(TypeError, match="VAEModel"):
        CL.clipping_profile(_svi(vae, VAEGuide(vae)), None, X)
    with pytest.raises(NotImplementedError, match="num_particles=3"):
        CL.gradient_norms(_svi(LogisticRegression(4), K=3), None, X, y)
    with pytest.raises(L.D3PError, match="2048"):
        CL.gradient_norms(_svi(PoissonRegression(2049)), None, np.zeros((2, 2049), np.float32), np.zeros(2, np.float32))
    good = _svi(LogisticRegression(4))
    for bad in ((0.0,), (-1.0,), (float("inf"),), (float("nan"),), (1e-60,), (1e60,), tuple(range(1, 10))):
        with pytest.raises(ValueError, match="threshold"):
            CL.clipping_profile(good, None, X, y, thresholds=bad)
        with pytest.raises(ValueError, match="threshold"):
            CL.norm_profile(torch.zeros(3), bad, (0.5,))
    for bad in ((-0.1,), (1.5,), (float("nan"),), tuple(i / 10 for i in range(9))):
        with pytest.raises(ValueError, match="prob"):
            CL.clipping_profile(good, None, X, y, probs=bad)
        with pytest.raises(ValueError, match="prob"):
            CL.norm_profile(torch.zeros(3), (1.0,), bad)
    with pytest.raises(ValueError, match="CUDA"):
        CL.norm_profile(torch.zeros(3), (1.0,), (0.5,))          # a CPU tensor
    with pytest.raises(ValueError, match="slab_bytes"):
        from d3p_amd.models import MeanFieldGuide
        sites_model = LogisticRegression(4, intercept=True)
        CL.gradient_norms(_svi(sites_model, MeanFieldGuide(sites_model)), None, X, y, slab_bytes=0)


def test_module_docstring_states_the_privacy_caveat():
    from d3p_amd import clipping as CL
    doc = " ".join(CL.__doc__.split())
    assert "PRIVATE table" in doc and "NOT covered by the accountant" in doc and "public or synthetic data" in doc


def test_public_surface():
    import d3p_amd
    from d3p_amd import _lib as L
    assert "clipping" in d3p_amd.__all__ and d3p_amd.clipping.ClippingProfile._fields == (
        "n", "n_nonfinite", "mean", "rms", "max", "probs", "quantiles", "thresholds", "clipped_fraction", "mean_clip_factor")
    for name in ("d3p_logreg_grad_norms_workspace", "d3p_logreg_grad_norms", "d3p_norm_profile_workspace", "d3p_norm_profile"):
        assert name in L.SIGNATURES
    assert any(p.endswith("d3p_grad_norms.hip") for p in L._SRC)


# ---------------------------------------------------------------- the calibration of the GPU tests' bound
@pytest.mark.parametrize("family", CR.FAMILIES)
def test_float32_calibration_stays_at_or_below_the_written_figures(O, family):
    """The float32 reference's own error over the inputs of the GPU sweep: at or below the figure the bound is four times of; and no
    row of the sweep has |t| > 20 (the Poisson inputs in particular)."""
    got, where, tmax = CR.float32_norm_calibration(O, family)
    print(f"{family}: smallest passing rtol {got:.3e} at (d, intercept, rows, guide, key noise) = {where}; written {CR.CALIBRATED[family]:.3e}; "
          f"max |t| {tmax:.2f}")
    assert 0.0 < got <= CR.CALIBRATED[family]
    assert CR.NORM_TOL[family] == 4 * CR.CALIBRATED[family]
    assert tmax <= 20.0
