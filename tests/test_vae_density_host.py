"""tests/vae_density_ref.py on its own (no GPU): the reference of the log importance weights against an independent evaluation, Jensen's
inequality of the importance-weighted bound, the brute-force column statistics against numpy, and the host-side checks of
d3p_amd.vae_density that run before the device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import predictive_ref as P
from tests import vae_density_ref as R


def _case(seed, D=37, Z=5, B=4, n=6, H=8, H2=0):
    rng = np.random.default_rng(seed)
    _, ldec, lenc, heads = P.vae_net(D, H, Z, H2, rng, scale=0.1)
    X = rng.random((B, D)).astype(np.float32)
    z = rng.normal(size=(n, B, Z)).astype(np.float32)
    return z, X, ldec, lenc, heads


@pytest.mark.parametrize("H2", [0, 4])
def test_parts_sum_to_log_w_and_match_an_independent_evaluation(H2):
    z, X, ldec, lenc, heads = _case(1, H2=H2)
    ref = R.log_weights_ref(z, X, ldec, lenc, heads)
    lw, px, pz, qz = (ref[k][0] for k in ("log_w", "log_px", "log_pz", "log_qz"))
    assert np.array_equal(lw, px + pz - qz)
    # independently: Bernoulli through the probabilities, the normals through their densities
    n, B, Z = z.shape
    zl, _, zs, _ = P.vae_encode_bound(X, lenc, heads)
    a, _ = P.vae_decode_bound(z.reshape(n * B, Z), ldec)
    p = P.expit(a.reshape(n, B, -1))
    x = X.astype(np.float64)[None]
    px2 = (x * np.log(p) + (1 - x) * np.log1p(-p)).sum(-1)
    z64 = z.astype(np.float64)
    pz2 = np.log(np.exp(-0.5 * z64 ** 2) / math.sqrt(2 * math.pi)).sum(-1)
    sd = np.exp(zs)[None]
    qz2 = np.log(np.exp(-0.5 * ((z64 - zl[None]) / sd) ** 2) / (sd * math.sqrt(2 * math.pi))).sum(-1)
    for got, want in ((px, px2), (pz, pz2), (qz, qz2)):
        assert np.all(np.abs(got - want) <= 1e-10 * (1 + np.abs(want)))
    for k in ref:
        assert ref[k][1].shape == (n, B) and np.all(ref[k][1] > 0) and np.all(np.isfinite(ref[k][1]))


def test_bound_vanishes_with_exact_heads():
    """Zero encoder heads: zl = zs = 0 exactly, so the log_qz bound is the float32 difference's alone."""
    z, X, ldec, lenc, heads = _case(2)
    for leaf in heads:
        leaf[...] = 0
    ref = R.log_weights_ref(z, X, ldec, lenc, heads)
    z64 = z.astype(np.float64)
    want = 2.0 ** -23 * (z64 ** 2).sum(-1)
    v, b = ref["log_qz"]
    assert np.allclose(b, want + 2.0 ** -24 * (np.abs(v) + want), rtol=1e-12, atol=0)
    assert np.array_equal(ref["log_pz"][0], ref["log_qz"][0])


def test_importance_weighted_bound_dominates_the_elbo():
    rng = np.random.default_rng(3)
    logw = (5 * rng.normal(size=(33, 7)) - 300).astype(np.float32)
    d, _ = R.density_from_logw(logw)
    assert np.all(d["log_px_is"] >= d["elbo"])
    assert np.all(d["log_px_is"] <= logw.max(0)) and np.all(d["ess"] >= 1) and np.all(d["ess"] <= 33)
    one, _ = R.density_from_logw(logw[:1])
    assert np.array_equal(one["log_px_is"], one["elbo"]) and np.array_equal(one["elbo"], logw[0].astype(np.float64))
    assert np.all(np.isnan(one["elbo_draw_var"])) and np.array_equal(one["ess"], np.ones(7))
    flat, _ = R.density_from_logw(np.full((9, 2), -12.5, np.float32))
    assert np.array_equal(flat["log_px_is"], flat["elbo"]) and np.allclose(flat["ess"], 9, rtol=1e-15) and np.array_equal(flat["elbo_draw_var"], np.zeros(2))


@pytest.mark.parametrize("n,cols", [(1, 1), (2, 33), (65, 3), (300, 5)])
def test_column_statistics_against_numpy(n, cols):
    rng = np.random.default_rng(n + cols)
    m = (rng.normal(size=(n, cols)) * rng.uniform(0.1, 30, cols) - rng.uniform(0, 500, cols)).astype(np.float32)
    ref, bnd = R.col_stats_ref(m)
    m64 = m.astype(np.float64)
    mx = m64.max(0)
    r = np.exp(m64 - mx)
    with np.errstate(invalid="ignore", divide="ignore"):
        got = {"mean": m64.mean(0), "var": m64.var(0, ddof=1) if n > 1 else np.full(cols, np.nan), "lse": mx + np.log(r.sum(0)) - math.log(n),
               "ess": r.sum(0) ** 2 / (r * r).sum(0)}
    # numpy's sums and exp are held to the bounds derived for the device's (pairwise sums are within the sequential bound; exp within 1 ulp)
    assert R.assert_col_stats(got, m, f"numpy n={n} cols={cols}") <= 1.0


def test_column_statistics_special_columns():
    m = np.zeros((4, 3), np.float32)
    m[:, 0] = [1, 2, np.nan, 3]
    m[:, 1] = -np.inf
    m[:, 2] = [0, -np.inf, 0, 0]
    ref, _ = R.col_stats_ref(m)
    assert all(np.isnan(ref[k][0]) for k in ref)
    assert ref["mean"][1] == -np.inf and ref["lse"][1] == -np.inf and np.isnan(ref["var"][1]) and np.isnan(ref["ess"][1])
    assert abs(ref["lse"][2] - math.log(3 / 4)) < 1e-15 and ref["ess"][2] == 3 and ref["mean"][2] == -np.inf


def test_host_checks_come_before_the_device():
    """Every refusal of the Python layer is raised without a GPU."""
    from d3p_amd import vae_density as VD
    from d3p_amd.models import AutoDiagonalNormal, LogisticRegression, VAEGuide, VAEModel
    lr = LogisticRegression(4)
    model = VAEModel(3, 8)
    X = np.zeros((2, 5), np.float32)
    for fn in (VD.log_importance_weights, VD.held_out_density):
        with pytest.raises(TypeError):
            fn(None, 4, lr, AutoDiagonalNormal(lr), {}, X)
        with pytest.raises(TypeError):
            fn(None, 4, model, AutoDiagonalNormal(lr), {}, X)
        with pytest.raises(ValueError):
            fn(None, 0, model, VAEGuide(model), {}, X)
        with pytest.raises(ValueError):
            fn(None, 4, model, VAEGuide(model), None, X)
    with pytest.raises(ValueError):
        VD.held_out_density(None, 65536, model, VAEGuide(model), {}, X)
    with pytest.raises(ValueError):
        VD.log_importance_weights(None, 2, model, VAEGuide(model), {}, X, multi=False)


def test_infer_util_still_refuses_the_vae():
    from d3p_amd import infer_util as U
    from d3p_amd.models import VAEModel
    with pytest.raises(TypeError):
        U.log_likelihood(VAEModel(3, 8), {}, np.zeros((2, 5), np.float32))


def test_workspace_is_sized_by_the_slab():
    import d3p_amd._lib as L
    lib = L.load()
    vm = L.VaeModel(784, 400, 50, 1.0, 1.0, 0)
    size = lambda B, k: int(lib.d3p_vae_log_weights_workspace(C.byref(vm), B, k))   # noqa: E731
    assert size(4096, 0) == 0 and size(0, 4) == 0
    s1, s2, s4 = size(4096, 1), size(4096, 2), size(4096, 4)
    assert 0 < s1 < s2 < s4
    per_draw = 4096 * (784 + 3 * 400) * 4
    assert s2 - s1 == per_draw and s4 - s2 == 2 * per_draw   # linear in the slab: nothing is sized by n
    # a small batch: a slab is never shorter than the 97 rows that keep every slab on one product kernel
    assert size(5, 1) == size(5, 20) < size(5, 21)
