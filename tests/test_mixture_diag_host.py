"""Host half of d3p_amd.mixture_diagnostics: tests/mixture_diag_ref.py against torch.distributions, the k = 1
closed form, xlogy at alpha_j == 1 with pis_j == 0, the module's own float64 densities against the reference on CPU tensors, every
refusal raised without a device, the exports, the entry points' declarations and the strip function."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import guide_diag_ref as G
from tests import mixture_diag_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53
SHAPES = [(1, 6), (3, 2), (5, 7), (16, 3)]     # (k, d)


def _mg(**kw):
    from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel
    m = GaussianMixtureModel(**kw)
    return m, GaussianMixtureGuide(m)


def _draws(k, d, n, seed):
    """float32 draws (pis (n, k), mus (n, k, d), sigs (n, k, d)) and params, of the guide's families."""
    r = np.random.default_rng([seed, k, d, n])
    alpha_log = (0.5 * r.normal(size=k)).astype(np.float32)
    mus_loc = (3.0 * r.normal(size=(k, d))).astype(np.float32)
    g = r.gamma(np.exp(alpha_log.astype(np.float64)), size=(n, k))
    pis = (g / g.sum(axis=1, keepdims=True)).astype(np.float32)
    mus = (mus_loc[None] + r.normal(size=(n, k, d))).astype(np.float32)
    sigs = (1.0 / r.gamma(1.0, size=(n, k, d))).astype(np.float32)
    return pis, mus, sigs, alpha_log, mus_loc


# ---------------------------------------------------------------- the reference against torch.distributions
@pytest.mark.parametrize("k,d", SHAPES)
def test_reference_densities_agree_with_torch_distributions(k, d):
    """Bound T 2^-53 sum |terms| with T the number of elementary terms of the density: a Normal site has three per element (the
    quadratic, log scale, log(2 pi) / 2), the Dirichlet k powers, k + 1 log-gammas, the InverseGamma two per element."""
    from torch.distributions import Dirichlet, Gamma, Normal
    n, tau = 9, 10.0
    pis, mus, sigs, alpha_log, mus_loc = _draws(k, d, n, 3)
    t = lambda a: torch.tensor(np.asarray(a, np.float32)).to(torch.float64)   # noqa: E731
    alpha = R.alpha_of(alpha_log)
    kd = k * d
    zero, one = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)

    def close(got, want, terms, mag, what):
        err = np.abs(np.asarray(got) - want)
        bound = terms * U53 * mag
        print(f"{what} k={k} d={d}: largest error / bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound), what

    want = Normal(zero, tau * one).log_prob(t(mus)).sum((1, 2)).numpy()
    close(R.log_p_mus(mus, tau), want, 3 * kd, R.log_p_mus_mag(mus, tau), "log p(mus)")
    want = Normal(t(mus_loc), one).log_prob(t(mus)).sum((1, 2)).numpy()
    close(R.log_q_mus(mus, mus_loc), want, 3 * kd, R.log_q_mus_mag(mus, mus_loc), "log q(mus)")
    # s ~ InverseGamma(1, 1)  <=>  1 / s ~ Gamma(1, 1):  log p(s) = Gamma(1, 1).log_prob(1 / s) - 2 log s
    s64 = t(sigs)
    want = (Gamma(one, one).log_prob(1.0 / s64) - 2.0 * torch.log(s64)).sum((1, 2)).numpy()
    close(R.log_p_sigs(sigs), want, 2 * kd, R.log_p_sigs_mag(sigs), "log p(sigs)")
    p64 = t(pis)
    p64 = p64 / p64.sum(1, keepdim=True)       # (the simplex in float64: Dirichlet's support check; the reference gets the same values)
    want = Dirichlet(torch.tensor(alpha)).log_prob(p64).numpy()
    close(R.log_q_pis(p64.numpy(), alpha), want, 2 * k + 1, np.maximum(R.log_q_pis_mag(p64.numpy(), alpha), 1e-300), "log q(pis)")
    want = Dirichlet(torch.ones(k, dtype=torch.float64)).log_prob(p64).numpy()
    assert np.all(np.abs(R.log_p_pis(k) - want) <= 4 * U53 * max(abs(math.lgamma(k)), 1.0))


def test_k_equal_one_closed_form():
    """k = 1: pis == 1, both Dirichlet terms are exactly 0, and log r_s = sum_r log N(x_r; mus_s, sigs_s) + log N(mus_s; 0, tau) -
    log N(mus_s; mus_loc, 1)."""
    from torch.distributions import Normal
    n, d, rows, tau = 7, 5, 40, 2.5
    _, mus, sigs, alpha_log, mus_loc = _draws(1, d, n, 11)
    pis = np.ones((n, 1), np.float32)
    assert R.log_p_pis(1) == 0.0 and np.all(R.log_q_pis(pis, R.alpha_of(alpha_log)) == 0.0)
    x = np.random.default_rng(5).normal(size=(rows, d)).astype(np.float32)
    t = lambda a: torch.tensor(np.asarray(a, np.float32)).to(torch.float64)   # noqa: E731
    lik = Normal(t(mus)[:, None, 0, :], t(sigs)[:, None, 0, :]).log_prob(t(x)[None]).sum((1, 2))
    totals = lik.numpy()
    prior = Normal(torch.zeros((), dtype=torch.float64), torch.tensor(tau, dtype=torch.float64)).log_prob(t(mus)).sum((1, 2)).numpy()
    q = Normal(t(mus_loc), torch.ones((), dtype=torch.float64)).log_prob(t(mus)).sum((1, 2)).numpy()
    want = totals + prior - q
    got = R.log_ratio(totals, 1, pis, mus, alpha_log, mus_loc, tau)
    bound = 3 * d * U53 * (R.log_p_mus_mag(mus, tau) + R.log_q_mus_mag(mus, mus_loc)) + 4 * U53 * (np.abs(totals) + np.abs(want))
    assert np.all(np.abs(got - want) <= bound)


def test_xlogy_at_alpha_one_with_a_zero_weight():
    """pis_j == 0: nothing at alpha_j == 1 (log q finite), +inf at alpha_j < 1, -inf at alpha_j > 1 -- reference and module alike."""
    from d3p_amd import mixture_diagnostics as MDG
    pis = np.array([[0.0, 0.25, 0.75], [0.5, 0.25, 0.25]], np.float32)
    for a0, want in ((1.0, None), (0.5, math.inf), (2.0, -math.inf)):
        alpha = np.array([a0, 1.5, 0.7])
        ref = R.log_q_pis(pis, alpha)
        got = MDG._log_q_pis(torch.tensor(pis).to(torch.float64), torch.tensor(alpha)).numpy()
        assert np.isfinite(ref[1]) and np.isfinite(got[1])
        if want is None:
            const = math.lgamma(3.2) - math.lgamma(1.0) - math.lgamma(1.5) - math.lgamma(0.7)
            exact = const + 0.5 * math.log(0.25) - 0.3 * math.log(0.75)
            assert abs(ref[0] - exact) <= 1e-14 and abs(got[0] - exact) <= 1e-14
        else:
            assert ref[0] == want and got[0] == want


@pytest.mark.parametrize("k,d", SHAPES)
def test_module_densities_match_the_reference_on_cpu_tensors(k, d):
    from d3p_amd import mixture_diagnostics as MDG
    n, tau = 6, 10.0
    pis, mus, sigs, alpha_log, mus_loc = _draws(k, d, n, 8)
    t = lambda a: torch.tensor(np.asarray(a, np.float32)).to(torch.float64)   # noqa: E731
    alpha = torch.exp(t(alpha_log))
    m2, s2 = t(mus).reshape(n, -1), t(sigs).reshape(n, -1)
    lp = MDG._log_p_pis(k) + MDG._log_p_mus(m2, tau)
    lq = MDG._log_q_pis(t(pis), alpha) + MDG._log_q_mus(m2, t(mus_loc).reshape(-1))
    zero = np.zeros(n)
    want = R.log_ratio(zero, k, pis, mus, alpha_log, mus_loc, tau)
    assert np.all(np.abs((lp - lq).numpy() - want) <= R.density_bound(k, d, pis, mus, sigs, alpha_log, mus_loc, tau, False))
    want = R.log_joint(zero, k, mus, sigs, tau)
    got = (lp + MDG._log_p_sigs(s2)).numpy()
    assert np.all(np.abs(got - want) <= R.density_bound(k, d, pis, mus, sigs, alpha_log, mus_loc, tau, True))


def test_tree_totals_is_a_reordering_of_the_row_sums():
    r = np.random.default_rng(2)
    for rows in (1, 63, 64, 65, 200, 2049 * 64 + 7):
        ll = (-50.0 * r.random((3, rows))).astype(np.float32)
        assert np.all(np.abs(R.tree_totals(ll) - G.totals(ll)) <= G.totals_bound(ll))
    assert R.tree_totals(np.zeros((4, 0), np.float32)).tolist() == [0.0] * 4
    one = np.array([[-1.25]], np.float32)
    assert R.tree_totals(one)[0] == -1.25


# ---------------------------------------------------------------- refusals, all without a device
def test_every_refusal_comes_without_a_device(monkeypatch):
    import d3p_amd._lib as L
    from d3p_amd import mixture_diagnostics as MDG
    from d3p_amd.models import AutoDiagonalNormal, LogisticRegression

    def no_device():
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(L, "require_device", no_device)
    m, g = _mg()
    k, d, rows = 3, 2, 10
    obs = np.zeros((rows, d), np.float32)
    params = {"alpha_log": np.zeros(k, np.float32), "mus_loc": np.zeros((k, d), np.float32)}
    key = torch.zeros(2, dtype=torch.uint32)          # (a CPU tensor: refused as a key, after everything else passed)
    run = lambda **kw: MDG.guide_diagnostic(kw.pop("key", key), kw.pop("n", 8), kw.pop("model", m), kw.pop("args", (k, obs)),   # noqa: E731
                                            kw.pop("guide", g), kw.pop("params", params), **kw)
    logreg = LogisticRegression(d)
    with pytest.raises(TypeError, match="GaussianMixtureModel"):
        run(model=logreg)
    with pytest.raises(TypeError, match="GaussianMixtureGuide"):
        run(guide=AutoDiagonalNormal(logreg))
    with pytest.raises(ValueError, match="obs is required"):
        run(args=(k, None, rows, d))
    with pytest.raises(ValueError, match="whole table"):
        run(args=(k, obs, rows + 1))
    with pytest.raises(ValueError, match="whole table"):
        run(num_obs_total=rows - 1)
    for n in (0, -3):
        with pytest.raises(ValueError, match="n must be >= 1"):
            run(n=n)
    with pytest.raises(ValueError, match="n must be >= 1"):
        run(n=None)
    with pytest.raises(ValueError, match="65535"):
        run(n=65536)
    for kk, dd in ((33, 2), (17, 129), (3, 257)):
        with pytest.raises(ValueError, match="supported shapes"):
            run(args=(kk, np.zeros((4, dd), np.float32)), params={"alpha_log": np.zeros(kk, np.float32), "mus_loc": np.zeros((kk, dd), np.float32)})
    with pytest.raises(ValueError, match="params"):
        run(params=[1, 2])
    with pytest.raises(ValueError, match="alpha_log"):
        run(params=dict(params, alpha_log=np.zeros(k + 1, np.float32)))
    with pytest.raises(ValueError, match="mus_loc"):
        run(params=dict(params, mus_loc=np.zeros((d, k), np.float32)))
    with pytest.raises(ValueError, match="prior_mu_scale"):
        run(model=_mg(prior_mu_scale=0.0)[0])
    with pytest.raises(TypeError, match="rng_key"):
        run()
    with pytest.raises(TypeError, match="rng_key"):
        run(key=None)
    # the sample-taking pair
    good = {"pis": np.full((4, k), 1.0 / k, np.float32), "mus": np.zeros((4, k, d), np.float32), "sigs": np.ones((4, k, d), np.float32)}
    for fn in (MDG.log_likelihood_total, MDG.log_joint):
        with pytest.raises(TypeError, match="GaussianMixtureModel"):
            fn(logreg, good, obs)
        with pytest.raises(ValueError, match="obs is required"):
            fn(m, good, None)
        with pytest.raises(ValueError, match="obs"):
            fn(m, good, np.zeros((rows, d + 1), np.float32))
        with pytest.raises(ValueError, match="posterior_samples"):
            fn(m, {"pis": good["pis"]}, obs)
        with pytest.raises(ValueError, match="leading draw axis"):
            fn(m, dict(good, pis=good["pis"][0]), obs)
        with pytest.raises(ValueError, match="mus"):
            fn(m, dict(good, mus=np.zeros((4, k + 1, d), np.float32)), obs)
        with pytest.raises(ValueError, match="supported shapes"):
            fn(m, {"pis": np.ones((2, 33), np.float32), "mus": np.zeros((2, 33, 2), np.float32), "sigs": np.ones((2, 33, 2), np.float32)}, obs)
    with pytest.raises(ValueError, match="prior_mu_scale"):
        MDG.log_joint(_mg(prior_mu_scale=-1.0)[0], good, obs)


def test_without_a_device_there_is_no_fallback(monkeypatch):
    import d3p_amd._lib as L
    from d3p_amd import mixture_diagnostics as MDG

    def no_device():
        raise L.D3PError("no device")
    monkeypatch.setattr(L, "require_device", no_device)
    m, _ = _mg()
    good = {"pis": np.full((4, 3), 1.0 / 3, np.float32), "mus": np.zeros((4, 3, 2), np.float32), "sigs": np.ones((4, 3, 2), np.float32)}
    for fn in (MDG.log_likelihood_total, MDG.log_joint):
        with pytest.raises(L.D3PError):
            fn(m, good, np.zeros((5, 2), np.float32))


# ---------------------------------------------------------------- surface
def test_exports_and_entry_points():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import diagnostics as DG
    from d3p_amd import mixture_diagnostics as MDG
    assert d3p_amd.mixture_diagnostics is MDG and "mixture_diagnostics" in d3p_amd.__all__
    assert MDG.__all__ == ["log_likelihood_total", "log_joint", "guide_diagnostic", "GuideDiagnostic"]
    assert MDG.GuideDiagnostic is DG.GuideDiagnostic
    # the top-level names keep pointing at the regression module
    assert d3p_amd.log_joint is DG.log_joint and d3p_amd.guide_diagnostic is DG.guide_diagnostic
    assert d3p_amd.log_likelihood_total is DG.log_likelihood_total
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint d3p_gmm_loglik_draw_sums\(", hdr) and re.search(r"\bsize_t d3p_gmm_loglik_draw_sums_workspace\(", hdr)
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    assert len(L.SIGNATURES["d3p_gmm_loglik_draw_sums"][1]) == 11 and len(L.SIGNATURES["d3p_gmm_loglik_draw_sums_workspace"][1]) == 4
    lib = L.load()
    assert lib.d3p_abi_version() == 9 and hasattr(lib, "d3p_gmm_loglik_draw_sums")
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "d3p_gmm_loglik_draw_sums" in f.read()
    with open(os.path.join(ROOT, "d3p_amd", "csrc", "d3p_gmm_density.hip")) as f:
        src = f.read()
    assert int(re.search(r"#define D3P_GD_MAX_STRIPS (\d+)", src).group(1)) == R.MAX_STRIPS
    assert int(re.search(r"#define D3P_GD_ROW_TILE (\d+)", src).group(1)) == R.TILE


def test_import_stays_lazy():
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.mixture_diagnostics' not in sys.modules; " \
           "d3p_amd.mixture_diagnostics; assert 'd3p_amd.mixture_diagnostics' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_strip_function_depends_on_rows_alone():
    import d3p_amd._lib as L
    lib = L.load()
    assert R.strips_of(0) == (0, 0) and R.strips_of(1) == (1, 1) and R.strips_of(64 * 2048) == (2048, 1)
    assert R.strips_of(64 * 2048 + 1) == (1025, 2) and R.strips_of(7000 * 64 + 5) == (1751, 4) and R.strips_of(10 ** 6) == (1954, 8)
    for rows in (0, 1, 64, 65, 64 * 2048, 64 * 2048 + 1, 7000 * 64 + 5, 10 ** 6, 10 ** 7):
        strips, per = R.strips_of(rows)
        assert strips <= R.MAX_STRIPS == 2048 and (rows == 0 or (strips - 1) * per * 64 < rows <= strips * per * 64)
        for n, d, k in ((1, 1, 1), (5, 2, 3), (128, 64, 16), (65535, 128, 32)):
            assert lib.d3p_gmm_loglik_draw_sums_workspace(rows, d, k, n) == 8 * strips * n, (rows, n)


def test_the_regression_module_still_refuses_the_mixture():
    from d3p_amd import diagnostics as DG
    m, g = _mg()
    x = np.zeros((4, 2), np.float32)
    with pytest.raises(TypeError, match="unsupported model GaussianMixtureModel"):
        DG.log_joint(m, {"pis": np.ones((1, 3), np.float32)}, x)
    with pytest.raises(TypeError, match="unsupported model GaussianMixtureModel"):
        DG.guide_diagnostic(torch.zeros(2, dtype=torch.uint32), 4, m, (x,), g, {})
