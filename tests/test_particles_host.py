"""Trace_ELBO(num_particles=K) on the host: argument validation, the refusals that come before any device call, and the new
C entry points' declarations.  No GPU needed."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["d3p_logreg_px_grads_particles_workspace", "d3p_logreg_px_grads_particles", "d3p_dpvi_logreg_local_sums_particles",
               "d3p_dpvi_logreg_run_particles_from", "d3p_logreg_evaluate_particles_workspace", "d3p_logreg_evaluate_particles",
               "d3p_logreg_evaluate_sites_particles", "d3p_px_eps_sites_particles"]


@pytest.mark.parametrize("k", [0, -1, 2.5, "2", True, None])
def test_trace_elbo_rejects_bad_particle_counts(k):
    from d3p_amd.models import Trace_ELBO
    with pytest.raises(ValueError):
        Trace_ELBO(num_particles=k)


@pytest.mark.parametrize("k", [1, 2, 4, 9])
def test_trace_elbo_accepts_positive_integers(k):
    import numpy as np
    from d3p_amd.models import Trace_ELBO
    assert Trace_ELBO(num_particles=k).num_particles == k
    assert Trace_ELBO(num_particles=np.int64(k)).num_particles == k
    assert Trace_ELBO(k, vectorize_particles=False).num_particles == k
    assert Trace_ELBO().num_particles == 1


def _gmm_svi(k):
    from d3p_amd.models import Adam, GaussianMixtureGuide, GaussianMixtureModel, Trace_ELBO
    from d3p_amd.svi import DPSVI
    model = GaussianMixtureModel(k=3)
    return DPSVI(model, GaussianMixtureGuide(model), Adam(1e-3), Trace_ELBO(num_particles=k), 1.0, 1.0, N=100)


def _vae_svi(k):
    from d3p_amd.models import Adam, Trace_ELBO, VAEGuide, VAEModel
    from d3p_amd.svi import DPSVI
    model = VAEModel(z_dim=4, hidden_dim=8)
    return DPSVI(model, VAEGuide(model), Adam(1e-3), Trace_ELBO(num_particles=k), 1.0, 1.0, N=100)


def _logreg_svi(k):
    from d3p_amd.models import Adam, AutoDiagonalNormal, LogisticRegression, Trace_ELBO
    from d3p_amd.svi import DPSVI
    model = LogisticRegression(8)
    return DPSVI(model, AutoDiagonalNormal(model), Adam(1e-3), Trace_ELBO(num_particles=k), 1.0, 1.0, N=100)


def test_mixture_model_and_vae_refuse_particles_at_construction(monkeypatch):
    import d3p_amd._lib as L

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(L, "require_device", no_device)
    with pytest.raises(NotImplementedError):
        _gmm_svi(2)
    with pytest.raises(NotImplementedError):
        _vae_svi(2)
    _gmm_svi(1)   # one particle stays what it was
    _vae_svi(1)
    assert _logreg_svi(3)._num_particles == 3


def test_data_parallel_engines_refuse_particles_before_the_device(monkeypatch):
    import d3p_amd._lib as L
    from d3p_amd import dist

    def no_device(*a, **k):
        raise AssertionError("the engine reached require_device")
    monkeypatch.setattr(L, "require_device", no_device)
    svi = _logreg_svi(2)
    for make in (lambda: dist.HipEngine(svi, None, None, 10, 0, 10, L.D3P_BATCH_FEISTEL, 4),
                 lambda: dist.FusedHipEngine(svi, None, None, 10, 0, 10, L.D3P_BATCH_FEISTEL, 4),
                 lambda: dist.VaeHipEngine(svi), lambda: dist.GmmHipEngine(svi)):
        with pytest.raises(NotImplementedError):
            make()


def test_new_entry_points_are_declared_and_bound():
    import d3p_amd._lib as L
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in L.SIGNATURES, name
    assert re.search(r"#define D3P_ABI_VERSION 9\b", header)


# ---------------------------------------------------------------- the comparator at K = 1 is the oracle's single-particle path
def test_comparator_eps_at_one_particle_is_the_oracles(O):
    from tests import particles_ref as R
    jk = O.convert_to_jax_rng_key(O.PRNGKey(5))
    assert np.array_equal(R.px_eps(O, jk, 6, 11, 1)[:, 0], O.px_eps(jk, 6, 11))
    assert np.array_equal(R.px_eps_sites(O, jk, 5, [7, 1], 1)[:, 0], O.px_eps_sites(jk, 5, [7, 1]))
    # the one-site guide's stream is the one-site case of the per-site rule, at every K
    assert np.array_equal(R.px_eps(O, jk, 4, 9, 3), R.px_eps_sites(O, jk, 4, [9], 3))


def test_comparator_evaluate_at_one_particle_is_the_oracles(O):
    from tests import particles_ref as R
    r = np.random.default_rng(3)
    d, B = 6, 9
    X = r.normal(size=(B, d)).astype(np.float32)
    y = (r.random(B) < 0.5).astype(np.float32)
    loc, unc = (0.3 * r.normal(size=d)).astype(np.float32), np.full(d, -1.0, np.float32)
    spec = O.logreg_spec(d, False, 1.0, 1.0, lik_scale=100, obs_scale=100)
    jk = O.convert_to_jax_rng_key(O.PRNGKey(8))
    assert R.evaluate(O, spec, loc, unc, X, y, jk, 1) == O.logreg_evaluate(spec, loc, unc, X, y, jk)


def test_comparator_update_at_one_particle_is_the_oracles(O):
    from tests import particles_ref as R
    r = np.random.default_rng(4)
    d, B, N = 5, 12, 200
    X = r.normal(size=(B, d)).astype(np.float32)
    y = (r.random(B) < 0.5).astype(np.float32)
    mask = (r.random(B) < 0.7).astype(np.float32)
    spec = O.logreg_spec(d, True, 1.0, 2.0, lik_scale=N, obs_scale=N)
    hy = O.Hyper(1.0, 0.8, 1e-2, 0.9, 0.999, 1e-8)
    D = d + 1
    a = O.LogregState(O.PRNGKey(2), D, np.zeros(D, np.float32), np.full(D, -2.0, np.float32))
    b = O.LogregState(O.PRNGKey(2), D, np.zeros(D, np.float32), np.full(D, -2.0, np.float32))
    for _ in range(3):
        la, ga = O.logreg_update(spec, hy, a, X, y, mask)
        lb, gb = R.update(O, spec, hy, b, X, y, 1, mask)
        np.testing.assert_allclose(lb, la, rtol=1e-6)
        np.testing.assert_allclose(gb, ga, rtol=1e-5, atol=1e-7 * np.abs(ga).max())
        assert np.array_equal(a.key, b.key)
    np.testing.assert_allclose(b.params, a.params, rtol=1e-5, atol=1e-7)
