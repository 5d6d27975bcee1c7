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


# ---------------------------------------------------------------- the K > 1 size limit (k_logreg_particles keeps the rows in LDS)
def _lds_limit(materialising):
    """The LDS arithmetic of csrc/d3p_logreg_particles.h restated: per wavefront (2 + 1 (+ 2 without materialising)) x D floats rounded
    down to a multiple of 4, plus 2 floats, at least one wavefront within 160 KB less 256 bytes."""
    def fits(D):
        wave = ((3 if materialising else 5) * D + 3) & ~3
        return (wave + 2) * 4 <= 160 * 1024 - 256
    D = 1
    while fits(D + 1):
        D += 1
    return D


def test_particle_limits_pinned_at_both_boundaries():
    import d3p_amd._lib as L
    lib = L.load()
    assert lib.d3p_logreg_particles_max_latent(0) == _lds_limit(False) == 8178
    assert lib.d3p_logreg_particles_max_latent(1) == _lds_limit(True) == 13630


def _model(L, D, icpt, N=100):
    return L.LogregModel(D - int(icpt), int(icpt), 1.0, 2.0, float(N), 1.0 / N, L.D3P_FAMILY_LOGREG, L.D3P_GUIDE_SOFTPLUS, 0.0)


def _scratch(nbytes):
    """(keep-alive, base address) of nbytes zeroed bytes: device memory where a device is visible (so that an entry which failed to
    refuse would run its kernels on real buffers, not fault on host addresses), else host memory (a launch then fails with D3P_E_HIP)."""
    import ctypes
    import torch
    if torch.cuda.is_available():
        t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        return t, t.data_ptr()
    host = (ctypes.c_uint8 * nbytes)()
    return host, ctypes.addressof(host)


@pytest.mark.parametrize("icpt", [False, True])
def test_c_entries_refuse_the_first_unsupported_size_before_any_launch(icpt):
    """At D = limit + 1 every K > 1 entry returns D3P_E_UNSUPPORTED naming the limit, before any launch.  Every pointer names its own
    1 MiB region of one zeroed buffer (larger than any array of these shapes) and the workspace its full size."""
    import ctypes
    import d3p_amd._lib as L
    lib = L.load()
    B = ctypes.byref
    h = L.DpsviHyper(1.0, 0.5, 1e-2, 0.9, 0.999, 1e-8)
    src = L.BatchSource(L.D3P_BATCH_EXPLICIT, 3, 0.0, 0, None, None, None, 3, 0, 3)
    m = _model(L, 8179, icpt)
    ws = lib.d3p_dpvi_logreg_workspace(B(m), B(src))
    keep, base = _scratch(ws + (16 << 20))
    r = [base + ws + (i << 20) for i in range(16)]   # regions after the workspace
    st = L.DpsviState(r[0], 0, r[1], r[2], r[3], r[4])
    rc = lib.d3p_dpvi_logreg_local_sums_particles(None, B(m), B(h), B(st), B(src), r[5], r[6], None, 2, r[7], base, ws)
    assert rc == -3 and b"8178" in lib.d3p_last_error(), lib.d3p_last_error()
    st2 = L.DpsviState(r[8], 0, r[9], r[10], r[11], r[12])
    rc = lib.d3p_dpvi_logreg_run_particles_from(None, B(m), B(h), B(st2), B(st), B(src), 0, r[5], r[6], 1, 3, r[7], base, ws)
    assert rc == -3 and b"8178" in lib.d3p_last_error(), lib.d3p_last_error()
    m = _model(L, 13631, icpt)
    ws2 = lib.d3p_logreg_px_grads_particles_workspace(B(m), 3, 2)
    assert ws2 <= ws
    rc = lib.d3p_logreg_px_grads_particles(None, B(m), r[1], r[5], r[6], None, 3, 2, None, r[0], r[7], r[8], r[9], base, ws2)
    assert rc == -3 and b"13630" in lib.d3p_last_error(), lib.d3p_last_error()
    del keep


def test_finalize_takes_the_sums_of_rows_wider_than_the_single_particle_forms():
    """d3p_dpvi_logreg_finalize launches no per-example kernel: at D = 6000 (the particle kernel's one-wavefront form; no single-particle
    form holds the rows) it does not refuse -- it runs on a device, and without one only the launch itself fails."""
    import ctypes
    import torch
    import d3p_amd._lib as L
    lib = L.load()
    B = ctypes.byref
    h = L.DpsviHyper(1.0, 0.5, 1e-2, 0.9, 0.999, 1e-8)
    src = L.BatchSource(L.D3P_BATCH_EXPLICIT, 3, 0.0, 0, None, None, None, 3, 0, 3)
    m = _model(L, 6000, False)
    ws = lib.d3p_dpvi_logreg_workspace(B(m), B(src))
    keep, base = _scratch(ws + (8 << 20))
    r = [base + ws + (i << 20) for i in range(8)]
    st = L.DpsviState(r[0], 0, r[1], r[2], r[3], r[4])
    rc = lib.d3p_dpvi_logreg_finalize(None, B(m), B(h), B(st), B(src), r[5], r[6], None, base, ws)
    assert b"latent dimension" not in lib.d3p_last_error()
    if torch.cuda.is_available():
        assert rc == 0, lib.d3p_last_error()
        torch.cuda.synchronize()
    else:
        assert rc == -2, (rc, lib.d3p_last_error())   # D3P_E_HIP: the launch
    del keep


@pytest.mark.parametrize("guide", ["auto", "meanfield", "sgd"])
def test_python_refusal_boundaries(monkeypatch, guide):
    """DPSVI._require_particle_rows: the last supported D passes, the next raises naming the limit; the stage follows the route
    (the staged composition -- here SGD -- materialises rows, the fused routes clip into sums).  No device is touched."""
    import d3p_amd._lib as L
    from d3p_amd.models import SGD, Adam, AutoDiagonalNormal, LogisticRegression, MeanFieldGuide, Trace_ELBO
    from d3p_amd.svi import DPSVI

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(L, "require_device", no_device)
    icpt = guide == "meanfield"
    for K in (1, 2, 5):
        model = LogisticRegression(8, intercept=icpt)
        g = MeanFieldGuide(model) if guide == "meanfield" else AutoDiagonalNormal(model)
        svi = DPSVI(model, g, SGD(1e-3) if guide == "sgd" else Adam(1e-3), Trace_ELBO(num_particles=K), 1.0, 1.0, N=100)
        materialising = svi._particle_route_materialises({})
        assert materialising == (guide == "sgd")
        limit = 13630 if materialising else 8178
        for stage, lim in ((materialising, limit), (True, 13630)):
            svi._require_particle_rows(lim - int(icpt), stage)
            if K == 1:
                svi._require_particle_rows(lim + 100, stage)      # one particle: no limit
                continue
            with pytest.raises(L.D3PError, match=str(lim)):
                svi._require_particle_rows(lim + 1 - int(icpt), stage)
