"""d3p_amd.diagnostics, host side: tests/guide_diag_ref.py against the closed forms of a linear regression on an orthogonal design,
the ordering of the Pareto k with the guide's quality, the module surface and the C entry's declaration, and every refusal of
log_likelihood_total / log_joint / guide_diagnostic before a device is touched."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import guide_diag_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_DRAWS, K_COLUMNS = 4096, 20


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("diagnostics reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


# ------------------------------------------------------------------------------------------------ the reference against closed forms
def _reference_ratios(prob, c, n, seed):
    """(lr, z, sum of the |terms| that enter one lr) of the reference on the guide Normal(m, c / sqrt(P))."""
    D = prob["m"].size
    z = np.random.default_rng([seed, n, D]).normal(size=(n, D))
    loc, sigma = G.scaled_posterior_guide(prob, c)
    theta = loc + sigma * z
    ll = G.linear_ll64(prob["X"], prob["y"], theta, G.ORTHO_SIGMA)
    lp = G.log_prior(theta, None, G.ORTHO_TAU, 1.0)
    lq = G.log_q(theta, loc, sigma)
    mag = np.abs(ll).sum(axis=1) + np.abs(G._normal_logpdf(theta, 0.0, G.ORTHO_TAU)).sum(axis=1) + np.abs(G._normal_logpdf(theta, loc, sigma)).sum(axis=1)
    return G.totals(ll) + lp - lq, z, mag


@pytest.mark.parametrize("D,rows", [(1, 64), (8, 257)])
def test_guide_equal_to_the_posterior_gives_the_log_evidence(D, rows):
    prob = G.orthogonal_problem(D, rows)
    Xt = prob["X"].astype(np.float64)
    off = Xt.T @ Xt - np.diag(prob["a"])
    assert not off.any()                                                # X^T X is exactly diagonal
    lr, _, mag = _reference_ratios(prob, 1.0, 64, 1)
    bound = rows * G.U53 * (mag + prob["ev_mag"])
    err = np.abs(lr - prob["log_evidence"])
    print(f"D={D} rows={rows}: largest error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    st = G.stats(lr)
    assert abs(st["elbo"] - prob["log_evidence"]) <= bound.max() and abs(st["log_evidence_is"] - st["elbo"]) <= 2.0 * bound.max()
    assert st["elbo_se"] <= 2.0 * bound.max() and abs(st["ess"] - 64.0) <= 64.0 * 8.0 * bound.max()
    same = np.full(64, lr[0])                                           # the ratios made exactly equal
    st = G.stats(same)
    assert st["elbo_se"] == 0.0 and st["log_evidence_is"] == st["elbo"] == lr[0] and st["ess"] == 64.0
    assert G.pareto_k(same) == -np.inf and G.pareto_k(same[:1]) == np.inf and G.pareto_k(lr[:20]) == np.inf


@pytest.mark.parametrize("c2", [0.5, 0.8, 1.5])
@pytest.mark.parametrize("D,rows", [(1, 64), (8, 257)])
def test_scaled_guide_follows_the_closed_form(D, rows, c2):
    c = math.sqrt(c2)
    prob = G.orthogonal_problem(D, rows)
    lr, z, mag = _reference_ratios(prob, c, 64, 2)
    want = prob["log_evidence"] + G.ratio_offsets(z, c)
    bound = rows * G.U53 * (mag + prob["ev_mag"] + np.abs(G.ratio_offsets(z, c)))
    err = np.abs(lr - want)
    print(f"D={D} rows={rows} c^2={c2}: largest error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    st = G.stats(lr)
    assert st["log_evidence_is"] >= st["elbo"] and st["elbo_se"] > 0.0 and 1.0 <= st["ess"] <= 64.0


def test_reference_special_values():
    lr = np.array([-3.0, -1.0, -2.0, -np.inf])
    st = G.stats(lr)
    assert st["elbo"] == -np.inf and np.isfinite(st["log_evidence_is"]) and G.pareto_k(lr) == np.inf
    assert abs(st["log_evidence_is"] - (np.log(np.exp(lr[:3]).sum()) - math.log(4))) <= 1e-15
    st = G.stats(np.full(3, -np.inf))
    assert st["elbo"] == -np.inf and st["log_evidence_is"] == -np.inf and G.pareto_k(np.full(3, -np.inf)) == np.inf
    lr[1] = np.nan
    assert all(np.isnan(v) for v in G.stats(lr).values()) and np.isnan(G.pareto_k(lr))
    assert np.isnan(G.stats(np.array([-1.0]))["elbo_se"]) and G.stats(np.array([-1.0]))["ess"] == 1.0
    want = np.array([0.0, 1.0e-3, 2.5, 40.0])                          # a large table: the shifted column keeps what float32 of lr loses
    col = G.k_column(-3.0e5 - want)
    assert col.dtype == np.float32 and col[0] == 0.0 and np.all(np.abs(col - want) <= 2.0 ** -24 * want + 3.0e5 * 2.0 ** -52)
    assert np.unique((-3.0e5 - want).astype(np.float32)).size < 4


# ------------------------------------------------------------------------------------------------ k-hat and the guide's quality
def _k_hats(D, c2):
    c = math.sqrt(c2)
    return np.array([G.pareto_k(G.ratio_offsets(np.random.default_rng([seed, D, K_DRAWS]).normal(size=(K_DRAWS, D)), c))
                     for seed in range(K_COLUMNS)])


@pytest.mark.parametrize("D", [1, 8])
def test_k_hat_orders_the_guides_by_their_tails(D):
    """The tail index of the ratios is 1 - c^2: the guide that is too narrow (c^2 = 0.5) has the heaviest tail, the one that is too
    wide (c^2 = 1.5) a bounded ratio.  Only the ordering of the means over 20 seeded columns of 4096 draws is asserted, and that the
    wide guide passes the threshold.  (Recorded means: D = 1: 0.47, 0.22, -1.71; D = 8: 0.63, 0.24, -0.21.)"""
    from d3p_amd.criteria import _k_threshold
    k = {c2: _k_hats(D, c2) for c2 in (0.5, 0.8, 1.5)}
    print({c2: (round(float(v.mean()), 3), round(float(v.std()), 3)) for c2, v in k.items()})
    assert all(np.isfinite(v).all() for v in k.values())
    assert k[0.5].mean() > k[0.8].mean() > k[1.5].mean()
    assert k[1.5].mean() < _k_threshold(K_DRAWS) and np.all(k[1.5] < _k_threshold(K_DRAWS))
    if D == 1:   # what tests/test_gpu_guide_diag.py's orthogonal case relies on: at D = 1 both guides lie below the threshold, column by column
        assert np.all(k[0.5] < _k_threshold(K_DRAWS)) and np.all(k[1.5] < 0.0) and np.all(k[0.5] > 0.0)


# ------------------------------------------------------------------------------------------------ surface
def test_module_surface_and_entry_points():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import diagnostics as DG
    for name in ("log_likelihood_total", "log_joint", "guide_diagnostic", "GuideDiagnostic"):
        assert getattr(d3p_amd, name) is getattr(DG, name) and name in d3p_amd.__all__ and name in DG.__all__
    assert DG.GuideDiagnostic._fields == ("elbo", "elbo_se", "log_evidence_is", "pareto_k", "k_threshold", "ess", "n_draws", "n_rows",
                                          "pointwise")
    assert any(os.path.basename(p) == "d3p_draw_sums.hip" for p in L._SRC) and all(p in L._DEPS for p in L._SRC)
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint d3p_loglik_draw_sums\(", hdr) and re.search(r"\bsize_t d3p_loglik_draw_sums_workspace\(", hdr)
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    assert len(L.SIGNATURES["d3p_loglik_draw_sums"][1]) == 13 and len(L.SIGNATURES["d3p_loglik_draw_sums_workspace"][1]) == 2
    lib = L.load()
    assert lib.d3p_abi_version() == 9 and hasattr(lib, "d3p_loglik_draw_sums")


def test_strip_count_is_a_function_of_the_rows_alone():
    """tiles = ceil(rows / 128); per = ceil(tiles / 512); strips = ceil(tiles / per); the workspace is 8 strips n bytes."""
    import d3p_amd._lib as L
    lib = L.load()

    def strips(rows):
        tiles = -(-rows // 128)
        per = -(-tiles // 512) if tiles else 0
        return -(-tiles // per) if tiles else 0
    for rows in (0, 1, 128, 129, 257, 65536, 65537, 131072, 131073, 10 ** 6, 10 ** 7, 2 ** 32 - 1):
        for n in (1, 100, 129):
            assert lib.d3p_loglik_draw_sums_workspace(rows, n) == 8 * strips(rows) * n, (rows, n)
    assert strips(65536) == 512 == max(strips(r) for r in range(1, 300000, 127)) and strips(131073) == 342 and strips(10 ** 6) == 489


def test_import_stays_lazy():
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.diagnostics' not in sys.modules; " \
           "d3p_amd.guide_diagnostic; assert 'd3p_amd.diagnostics' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_the_device(no_device):
    from d3p_amd import diagnostics as DG
    from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, GaussianMean, GaussianMixtureGuide, GaussianMixtureModel,
                                LinearRegression, LogisticRegression, MeanFieldGuide, PoissonRegression, VAEModel)
    X, y = np.zeros((6, 3), np.float32), np.zeros(6, np.float32)
    good = {"w": np.zeros((4, 3), np.float32)}
    key = torch.zeros(2, dtype=torch.int32)                                            # (a CPU tensor: the key check is the last)
    for bad_model in (GaussianMean(3), GaussianMixtureModel(), VAEModel(2, 4)):
        for fn in (DG.log_likelihood_total, DG.log_joint):
            with pytest.raises(TypeError, match="LogisticRegression, LinearRegression and PoissonRegression"):
                fn(bad_model, good, X, y)
        with pytest.raises(TypeError, match="LogisticRegression, LinearRegression and PoissonRegression"):
            DG.guide_diagnostic(key, 4, bad_model, (X, y), None, {})
    for model in (LogisticRegression(3), LinearRegression(3), PoissonRegression(3)):
        guide = AutoDiagonalNormal(model)
        params = {"auto_loc": np.zeros(3, np.float32), "auto_scale": np.ones(3, np.float32)}
        for fn in (DG.log_likelihood_total, DG.log_joint):
            with pytest.raises(ValueError, match="whole table"):
                fn(model, good, X, y, 7)                                               # N != rows
            with pytest.raises(ValueError, match="y is missing"):
                fn(model, good, X)
            with pytest.raises(ValueError):
                fn(model, good)
            with pytest.raises(ValueError, match="'w' is missing"):
                fn(model, {"intercept": np.zeros(4)}, X, y)
            with pytest.raises(ValueError, match="shape"):
                fn(model, {"w": np.zeros((4, 2), np.float32)}, X, y)
            with pytest.raises(ValueError, match="labels expected"):
                fn(model, good, X, y[:5])
        with pytest.raises(ValueError, match="intercept"):
            DG.log_joint(type(model)(3, intercept=True), good, X, y)
        with pytest.raises(ValueError, match="values expected"):
            DG.log_joint(type(model)(3, intercept=True), {"w": good["w"], "intercept": np.zeros(3)}, X, y)
        with pytest.raises(TypeError, match="guide"):
            DG.guide_diagnostic(key, 4, model, (X, y), GaussianMixtureGuide(GaussianMixtureModel()), params)
        with pytest.raises(ValueError, match="whole table"):
            DG.guide_diagnostic(key, 4, model, (X, y, 60), guide, params)
        for bad_n in (0, -3):
            with pytest.raises(ValueError, match="n must be >= 1"):
                DG.guide_diagnostic(key, bad_n, model, (X, y), guide, params)
        with pytest.raises(ValueError, match="65535"):
            DG.guide_diagnostic(key, 65536, model, (X, y), guide, params)
        with pytest.raises(ValueError, match="dict"):
            DG.guide_diagnostic(key, 4, model, (X, y), guide, [1.0, 2.0])
        with pytest.raises(ValueError, match="auto_scale"):
            DG.guide_diagnostic(key, 4, model, (X, y), guide, {"auto_loc": np.zeros(3, np.float32)})
        with pytest.raises(ValueError, match="values expected"):
            DG.guide_diagnostic(key, 4, model, (X, y), guide, {"auto_loc": np.zeros(4, np.float32), "auto_scale": np.ones(3, np.float32)})
        with pytest.raises(ValueError, match="y is missing"):
            DG.guide_diagnostic(key, 4, model, (X,), guide, params)
        with pytest.raises(TypeError, match="rng_key"):
            DG.guide_diagnostic(key, 4, model, (X, y, 6), guide, params)               # every host check passed: the key is refused
        with pytest.raises(TypeError, match="rng_key"):
            DG.guide_diagnostic(key, 4, model, (X, y), DiagonalNormalGuide(model, site="w"),
                                {"w_loc": np.zeros(3, np.float32), "w_std_log": np.zeros(3, np.float32)})
    # the two-site guide is the logistic example's own: refused for the other families
    with pytest.raises(TypeError, match="guide"):
        DG.guide_diagnostic(key, 4, PoissonRegression(3, intercept=True), (X, y), MeanFieldGuide(LogisticRegression(3, intercept=True)), {})
