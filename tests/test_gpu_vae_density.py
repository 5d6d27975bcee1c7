"""d3p_amd.vae_density on the GPU: the log importance weights and their parts against the float64 reference with its derived bounds
(tests/vae_density_ref.py), the key rule, slab independence and determinism, the column statistics, the Pareto k, a closed form,
saturation, NaN containment, the refusals and the example's --held-out-density report.

Largest error / bound ratios observed (docs/experiments_vae_density.md has the table): every one is printed by the test that asserts
it."""
import argparse
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from d3p_amd import modelling as M
from d3p_amd import vae_density as VD
from d3p_amd.models import AutoDiagonalNormal, LogisticRegression, VAEGuide, VAEModel
from tests import predictive_ref as P
from tests import vae_density_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(t):
    return t.detach().cpu().numpy()


def _images(rng, B, D, kind):
    return (rng.random((B, D)) < 0.3).astype(np.float32) if kind == "binary" else rng.random((B, D)).astype(np.float32)


def _net(D, hid, Z, rng, scale=0.1):
    H, H2 = (hid, 0) if isinstance(hid, int) else hid
    tree, ldec, lenc, heads = P.vae_net(D, H, Z, H2, rng, scale=scale)
    model = VAEModel(Z, hid)
    return model, VAEGuide(model), tree, ldec, lenc, heads


def _check_all(lw, sites, X, ldec, lenc, heads, what):
    ref = R.log_weights_ref(_np(sites["z"]), X, ldec, lenc, heads)
    worst = R.assert_within(_np(lw), *ref["log_w"], f"{what} log_w")
    for k in ("log_px", "log_pz", "log_qz"):
        worst = max(worst, R.assert_within(_np(sites[k]), *ref[k], f"{what} {k}"))
    return worst


# ------------------------------------------------------------------------------- 1. sweep against the reference
@pytest.mark.parametrize("hid", [8, (8, 4)], ids=["h8", "h8_4"])
@pytest.mark.parametrize("Z", [3, 50])
@pytest.mark.parametrize("D", [37, 64, 784])
def test_sweep_against_reference(gpu, D, Z, hid):
    rng = np.random.default_rng(1000 * D + 10 * Z + (0 if isinstance(hid, int) else 1))
    model, guide, tree, ldec, lenc, heads = _net(D, hid, Z, rng)
    worst = 0.0
    for B in (1, 5, 67):
        for n in (1, 2, 33):
            for kind in ("binary", "uniform"):
                X = _images(rng, B, D, kind)
                lw, sites = VD.log_importance_weights(P.key(B + n), n, model, guide, tree, X, return_sites=True)
                assert tuple(lw.shape) == (n, B) and lw.dtype == torch.float32 and tuple(sites["z"].shape) == (n, B, Z)
                worst = max(worst, _check_all(lw, sites, X, ldec, lenc, heads, f"D={D} Z={Z} hid={hid} B={B} n={n} {kind}"))
    print(f"sweep D={D} Z={Z} hid={hid}: largest error / bound = {worst:.3g}")


# ------------------------------------------------------------------------------- 2. key rule and determinism
def test_z_is_the_posterior_predictive_z(gpu):
    rng = np.random.default_rng(2)
    D, Z, B, n = 64, 50, 5, 33
    model, guide, tree, *_ = _net(D, 8, Z, rng)
    X = _images(rng, B, D, "binary")
    key = P.key(7)
    _, sites = VD.log_importance_weights(key, n, model, guide, tree, X, return_sites=True)
    res = M.sample_multi_posterior_predictive(key, n, model, (B, Z, 8, D), guide, (X, Z, 8), tree)
    assert torch.equal(sites["z"], res["z"])
    _, one = VD.log_importance_weights(key, 1, model, guide, tree, X, multi=False, return_sites=True)
    single = M.sample_posterior_predictive(key, model, (B, Z, 8, D), guide, (X, Z, 8), tree)
    assert torch.equal(one["z"][0], single["z"])


@pytest.mark.parametrize("D,Z,hid,B,n", [(64, 50, 8, 67, 33), (784, 50, (8, 4), 67, 33), (37, 3, 8, 5, 33), (64, 8, 8, 128, 7)])
def test_outputs_do_not_depend_on_the_slab(gpu, D, Z, hid, B, n):
    rng = np.random.default_rng(3)
    model, guide, tree, *_ = _net(D, hid, Z, rng)
    X = _images(rng, B, D, "uniform")
    key = P.key(11)
    runs = [VD.log_importance_weights(key, n, model, guide, tree, X, return_sites=True, draws_per_slab=s) for s in (1, 3, n, n)]
    runs.append(VD.log_importance_weights(key, n, model, guide, tree, X, return_sites=True, max_workspace_bytes=1))   # the cap picks slab 1
    lw0, s0 = runs[0]
    for lw, s in runs[1:]:
        assert torch.equal(lw, lw0)
        for k in ("z", "log_px", "log_pz", "log_qz"):
            assert torch.equal(s[k], s0[k]), k
    assert torch.equal(VD.log_importance_weights(key, n, model, guide, tree, X), lw0)   # without the parts


def test_log_w_is_the_float64_combination_of_the_parts(gpu):
    """The kernel rounds (px + pz) - qz of its float64 sums once, and each part once: recombining the ROUNDED parts in float64 moves the
    value by at most half a float32 ulp of each part, and the two float32 roundings by half an ulp of log_w each."""
    rng = np.random.default_rng(4)
    D, Z, B, n = 784, 50, 67, 33
    model, guide, tree, *_ = _net(D, 8, Z, rng)
    X = _images(rng, B, D, "binary")
    lw, s = VD.log_importance_weights(P.key(1), n, model, guide, tree, X, return_sites=True)
    px, pz, qz = (s[k].double() for k in ("log_px", "log_pz", "log_qz"))
    comb = (px + pz) - qz
    tol = 2.0 ** -24 * (px.abs() + pz.abs() + qz.abs()) + 2.0 ** -23 * comb.abs()
    err = (lw.double() - comb).abs()
    print(f"log_w vs recombined parts: largest error / bound = {float((err / tol).max()):.3g}")
    assert bool((err <= tol).all())


# ------------------------------------------------------------------------------- 3. column statistics
def _stats_dict(m):
    mean, var, lse, ess = VD.col_stats(m)
    return {"mean": _np(mean), "var": _np(var), "lse": _np(lse), "ess": _np(ess)}


@pytest.mark.parametrize("cols", [1, 33])
@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_col_stats_against_float64(gpu, n, cols):
    rng = np.random.default_rng(100 * n + cols)
    ld = cols + 7
    buf = torch.tensor((rng.normal(size=(n, ld)) * rng.uniform(0.1, 30, ld) - rng.uniform(0, 500, ld)).astype(np.float32), device="cuda")
    m = buf[:, :cols]
    assert m.stride(0) == ld or n == 1
    R.assert_col_stats(_stats_dict(m), _np(m), f"col stats n={n} cols={cols}")


def test_col_stats_special_columns_leave_their_neighbours_alone(gpu):
    rng = np.random.default_rng(5)
    n, cols = 65, 33
    clean = torch.tensor((3 * rng.normal(size=(n, cols)) - 80).astype(np.float32), device="cuda")
    base = _stats_dict(clean)
    bad = clean.clone()
    bad[17, 4] = math.nan
    bad[:, 20] = -math.inf
    got = _stats_dict(bad)
    keep = np.ones(cols, bool)
    keep[[4, 20]] = False
    for k in base:
        assert np.array_equal(got[k][keep], base[k][keep]), k
        assert np.isnan(got[k][4])
    assert got["lse"][20] == -math.inf and np.isnan(got["ess"][20]) and got["mean"][20] == -math.inf and np.isnan(got["var"][20])
    R.assert_col_stats(got, _np(bad), "special columns")


# ------------------------------------------------------------------------------- 4. held_out_density and the Pareto k
def _psis_k(logw):
    import d3p_amd._lib as L
    n, B = logw.shape
    neg = (-logw).contiguous()
    out = torch.empty((3, B), dtype=torch.float32, device=logw.device)
    L.check(L.load().d3p_psis_loo(L.stream_ptr(), L.ptr(neg), B, n, B, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2])))
    return out[2].double()


def test_held_out_density_fields_and_pareto_k(gpu):
    rng = np.random.default_rng(6)
    D, Z, B, n = 64, 3, 5, 64
    model, guide, tree, *_ = _net(D, 8, Z, rng, scale=0.3)
    X = _images(rng, B, D, "binary")
    key = P.key(3)
    res = VD.held_out_density(key, n, model, guide, tree, X)
    lw = VD.log_importance_weights(key, n, model, guide, tree, X)
    assert (res.n_draws, res.n_images) == (n, B) and res.k_threshold == min(1 - 1 / math.log10(n), 0.7)
    ref, bnd = R.density_from_logw(_np(lw))
    for k in ref:
        got = _np(getattr(res, k))
        assert got.dtype == np.float64 and np.all(np.abs(got - ref[k]) <= bnd[k]), k
    assert np.all(_np(res.log_px_is) >= _np(res.elbo))   # Jensen
    k_direct = _psis_k(lw)
    assert torch.equal(res.pareto_k, k_direct) and bool(torch.isfinite(res.pareto_k).all())
    assert int(res.n_high_k) == int((~(k_direct <= res.k_threshold)).sum())
    e, l = _np(res.elbo), _np(res.log_px_is)
    assert abs(float(res.elbo_total) - e.sum()) <= 1e-12 * np.abs(e).sum()
    assert abs(float(res.log_px_is_total) - l.sum()) <= 1e-12 * np.abs(l).sum()
    assert abs(float(res.elbo_total_se) - math.sqrt(B * e.var(ddof=1))) <= 1e-9 * float(res.elbo_total_se)
    assert abs(float(res.log_px_is_total_se) - math.sqrt(B * l.var(ddof=1))) <= 1e-9 * float(res.log_px_is_total_se)
    # 16 draws leave no tail of five: +inf, and every image counts as high; pareto_k=False skips the fit
    few = VD.held_out_density(key, 16, model, guide, tree, X)
    assert bool(torch.isposinf(few.pareto_k).all()) and int(few.n_high_k) == B
    off = VD.held_out_density(key, 16, model, guide, tree, X, pareto_k=False)
    assert off.pareto_k is None and off.n_high_k is None and torch.equal(off.elbo, few.elbo)
    one = VD.held_out_density(key, 1, model, guide, tree, X[:1])
    assert math.isnan(float(one.elbo_total_se)) and math.isnan(float(one.log_px_is_total_se)) and math.isnan(float(one.elbo_draw_var[0]))
    assert torch.equal(one.elbo, one.log_px_is)   # one draw: logsumexp - log 1 is the draw itself
    with pytest.raises(ValueError):
        VD.held_out_density(key, 65536, model, guide, tree, X)


# ------------------------------------------------------------------------------- 5. closed form, saturation, NaN
def test_closed_form_guide_equal_to_prior(gpu):
    """First decoder weight and the four encoder head leaves zero: q = prior = Normal(0, 1) and p(x | z) does not see z, so every
    log_w[i, b] = c_b = sum_c x a_c - softplus(a_c) with a from the biases alone."""
    rng = np.random.default_rng(7)
    D, Z, B, n = 37, 50, 5, 33
    model, guide, tree, ldec, lenc, heads = _net(D, 8, Z, rng, scale=0.5)
    ldec[0][0][...] = 0
    for leaf in heads:
        leaf[...] = 0
    X = _images(rng, B, D, "uniform")
    key = P.key(9)
    lw, sites = VD.log_importance_weights(key, n, model, guide, tree, X, return_sites=True)
    ref = R.log_weights_ref(_np(sites["z"]), X, ldec, lenc, heads)
    a = P.softplus(ldec[0][1].astype(np.float64)) @ ldec[1][0].astype(np.float64) + ldec[1][1].astype(np.float64)
    c = (X.astype(np.float64) * a - P.softplus(a)).sum(-1)
    assert np.all(np.abs(ref["log_w"][0] - c[None]) <= 1e-9 * np.abs(c)[None])   # the reference agrees with the closed form
    R.assert_within(_np(lw), np.broadcast_to(c, (n, B)).copy(), ref["log_w"][1], "closed form log_w")
    res = VD.held_out_density(key, n, model, guide, tree, X, pareto_k=False)
    bound = ref["log_w"][1].max(0)
    d, b = R.density_from_logw(_np(lw))
    assert np.all(np.abs(_np(res.elbo) - c) <= bound) and np.all(np.abs(_np(res.log_px_is) - c) <= bound)
    assert np.all(np.abs(_np(res.log_px_is) - _np(res.elbo)) <= 2 * bound)
    # ess = n when every weight is equal; with weights spread over [c - bound, c + bound] it is at least n / cosh(2 bound)^2 >= n (1 - 4 bound^2)
    assert np.all(np.abs(_np(res.ess) - d["ess"]) <= b["ess"])
    assert np.all(np.abs(_np(res.ess) - n) <= b["ess"] + 4 * n * bound ** 2)


def test_saturated_logits_stay_finite(gpu):
    rng = np.random.default_rng(8)
    D, Z, B, n = 64, 3, 5, 2
    model, guide, tree, ldec, lenc, heads = _net(D, 8, Z, rng)
    X = _images(rng, B, D, "binary")
    X[0] = np.arange(D) % 2
    ldec[-1][1][...] = np.where(X[0] > 0, -60.0, 60.0)   # against the pixels of image 0
    lw, sites = VD.log_importance_weights(P.key(1), n, model, guide, tree, X, return_sites=True)
    assert bool(torch.isfinite(lw).all()) and float(lw[:, 0].max()) < -59.0 * D
    _check_all(lw, sites, X, ldec, lenc, heads, "saturated")


def test_nan_image_stays_in_its_column(gpu):
    rng = np.random.default_rng(9)
    D, Z, B, n = 64, 50, 67, 33
    model, guide, tree, *_ = _net(D, 8, Z, rng)
    X = _images(rng, B, D, "binary")
    key = P.key(2)
    clean = VD.held_out_density(key, n, model, guide, tree, X)
    lw0 = VD.log_importance_weights(key, n, model, guide, tree, X)
    X[13, 5] = math.nan
    lw = VD.log_importance_weights(key, n, model, guide, tree, X)
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[13] = False
    assert bool(torch.isnan(lw[:, 13]).all()) and torch.equal(lw[:, keep], lw0[:, keep])
    res = VD.held_out_density(key, n, model, guide, tree, X)
    for k in ("elbo", "elbo_draw_var", "log_px_is", "ess", "pareto_k"):
        got, was = getattr(res, k), getattr(clean, k)
        assert bool(torch.isnan(got[13])) and torch.equal(got[keep], was[keep]), k
    assert math.isnan(float(res.elbo_total)) and int(res.n_high_k) == int(clean.n_high_k) + (1 if float(clean.pareto_k[13]) <= clean.k_threshold else 0)


# ------------------------------------------------------------------------------- 6. refusals
def test_wrong_model_or_guide(gpu):
    rng = np.random.default_rng(10)
    model, guide, tree, *_ = _net(37, 8, 3, rng)
    X = _images(rng, 5, 37, "binary")
    lr = LogisticRegression(37)
    for fn in (VD.log_importance_weights, VD.held_out_density):
        with pytest.raises(TypeError):
            fn(P.key(0), 4, lr, AutoDiagonalNormal(lr), tree, X)
        with pytest.raises(TypeError):
            fn(P.key(0), 4, model, AutoDiagonalNormal(lr), tree, X)
    with pytest.raises(ValueError):
        VD.log_importance_weights(P.key(0), 0, model, guide, tree, X)


def test_entry_refuses_before_any_launch(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    rng = np.random.default_rng(11)
    D, Z, B, n = 37, 3, 5, 4
    model, guide, tree, *_ = _net(D, 8, Z, rng)
    vm = L.VaeModel(D, 8, Z, 1.0, 1.0, 0)
    flat = M._vae_flat_params(tree, vm, ("decoder$params", "encoder$params")).cuda()
    X = torch.tensor(_images(rng, B, D, "binary"), device="cuda")
    key = P.key(0)
    need = int(lib.d3p_vae_log_weights_workspace(C.byref(vm), B, n))
    assert need > 0 and int(lib.d3p_vae_log_weights_workspace(C.byref(vm), B, 0)) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    z = torch.full((n, B, Z), 7.0, device="cuda")
    lw = torch.full((n, B), 7.0, device="cuda")
    host = torch.zeros((n, B))

    def call(X_=X, lw_=lw, nbytes=need, dps=n, n_=n):
        return lib.d3p_vae_log_weights(L.stream_ptr(), C.byref(vm), L.ptr(flat), L.ptr(X_), B, L.ptr(key), n_, 1, dps, L.ptr(z), L.ptr(lw_), None,
                                       L.ptr(ws), nbytes)

    assert call(nbytes=need - 1) == -4            # D3P_E_WORKSPACE
    assert call(lw_=host) == -1                   # D3P_E_INVALID_ARG: a host pointer
    assert call(X_=host) == -1
    assert call(dps=0) == -1 and call(n_=0) == -1
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((lw == 7.0).all())   # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((lw == 7.0).any())
    out = torch.empty((4, 3), dtype=torch.float64, device="cuda")
    m = torch.zeros((2, 3), device="cuda")
    assert lib.d3p_col_stats(L.stream_ptr(), L.ptr(m), 2, 2, 3, L.ptr(out)) == -1          # ld < cols
    assert lib.d3p_col_stats(L.stream_ptr(), L.ptr(m), 3, 0, 3, L.ptr(out)) == -1          # no draws
    assert lib.d3p_col_stats(L.stream_ptr(), L.ptr(torch.zeros((2, 3))), 3, 2, 3, L.ptr(out)) == -1   # a host pointer


# ------------------------------------------------------------------------------- 7. the example's report
def test_example_reports_the_held_out_density(gpu, capsys):
    spec = importlib.util.spec_from_file_location("ex_vae_density", os.path.join(ROOT, "examples", "vae.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = argparse.Namespace(num_epochs=1, learning_rate=3e-3, batch_size=128, z_dim=50, hidden_dim=400, num_samples=512, sigma=0.01,
                              held_out_density=32)
    errs = mod.main(args)
    assert len(errs) == 1
    text = capsys.readouterr().out
    m = re.search(r"held-out density \(32 draws, (\d+) images\): ELBO per image = (\S+), IWAE bound per image = (\S+) \+- (\S+), "
                  r"n_high_k = (\d+)", text)
    assert m, text
    images, elbo, iwae, se, high = int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4)), int(m.group(5))
    assert images == 512 and all(math.isfinite(v) for v in (elbo, iwae, se)) and iwae >= elbo and 0 <= high <= images
