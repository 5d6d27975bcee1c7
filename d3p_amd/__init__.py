"""d3p_amd -- MI355X-native drop-in for the DP-VI update path of DPBayes/d3p.

Host Python mirrors d3p's public surface for that path (``d3p_amd.svi.DPSVI``, the ``rng_suite``
modules ``d3p_amd.random`` / ``d3p_amd.random.debug``, the batchifiers in ``d3p_amd.minibatch``)
and drives hand-written gfx950 kernels through the C-ABI of ``libd3p_hip.so`` (include/d3p_hip.h).
PyTorch is used for device memory, streams and torch.distributed only.
"""
from .version import __version__  # noqa: F401

__all__ = ["infer_util", "prediction", "predictive", "mixture", "mixture_density", "criteria", "loo", "posterior_loo", "LOOResult",
           "diagnostics", "log_likelihood_total", "log_joint", "guide_diagnostic", "GuideDiagnostic", "mixture_diagnostics", "intervals", "clipping",
           "scoring", "model_weights", "ppc", "discrepancy", "classification", "permutation", "marginals", "fidelity", "energy"]


def __getattr__(name):
    # d3p_amd.infer_util (log_likelihood, log predictive densities), d3p_amd.prediction (posterior predictive mean and variance) and
    # d3p_amd.predictive (predictive sampling for the regression family) and d3p_amd.mixture (predictive sampling and cluster
    # assignment for the mixture model) and d3p_amd.mixture_density (log predictive density and responsibilities of the mixture model)
    # and d3p_amd.criteria (waic, posterior_waic, compare) and d3p_amd.diagnostics (whole-table log joint, ELBO and the Pareto k of a
    # guide) and d3p_amd.mixture_diagnostics (the same for the mixture model's guide) and d3p_amd.intervals (credible and predictive
    # intervals, equal-tailed or highest-density, per-column quantiles, the latent summary) and d3p_amd.clipping (whole-table per-example gradient norms and the
    # clipping profile) and d3p_amd.scoring (CRPS and PIT calibration of predictive draws) and d3p_amd.model_weights (stacking and
    # pseudo-BMA(+) weights of M models, the comparison table) and d3p_amd.ppc (posterior predictive checks: per-draw statistics of
    # replicated data sets over their rows) and d3p_amd.discrepancy (realized-discrepancy chi-square checks and the Bayesian R^2) and
    # d3p_amd.classification (confusion counts per draw, ROC histogram, AUC and calibration of a logistic regression) and d3p_amd.energy
    # (the energy score of multivariate predictive draws) and d3p_amd.fidelity (energy distance and nearest-record checks of a synthetic
    # table) and d3p_amd.marginals (binned one- and two-way marginal fidelity of a synthetic table) and d3p_amd.permutation (the permutation test of
    # the energy distance) without making `import d3p_amd` import torch
    if name in ("infer_util", "prediction", "predictive", "mixture", "mixture_density", "criteria", "diagnostics", "mixture_diagnostics",
                "intervals", "clipping", "scoring", "model_weights", "ppc", "discrepancy", "classification", "energy", "fidelity", "marginals", "permutation"):
        import importlib
        return importlib.import_module("." + name, __name__)
    if name in ("loo", "posterior_loo", "LOOResult"):   # PSIS-LOO (d3p_amd.criteria), under the same lazy rule
        import importlib
        return getattr(importlib.import_module(".criteria", __name__), name)
    if name in ("log_likelihood_total", "log_joint", "guide_diagnostic", "GuideDiagnostic"):   # d3p_amd.diagnostics, likewise
        import importlib
        return getattr(importlib.import_module(".diagnostics", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
