"""d3p_amd.mixture_density on the GPU against tests/mixture_density_ref.py (the calibrated bound, the slack and the intervals are
stated there): all three outputs at every shape, row edge and draw edge on both input kinds, the rows form against the reduced form,
n = 1 against mixture.assignment_log_posterior, the posterior_* functions against the explicit path bit for bit, special values,
canaries, views of obs, the C entries' refusals and the example's opt-in flag."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from . import mixture_density_ref as D
from . import mixture_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, DT = D.T, D.DT
ALL_CASES = list(dict.fromkeys(D.CASES))


@pytest.fixture(scope="module")
def MD(gpu):
    from d3p_amd import mixture_density
    return mixture_density


def _mg():
    from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel
    m = GaussianMixtureModel()
    return m, GaussianMixtureGuide(m)


def _samples(ref):
    return {name: np.array(ref[name]) for name in ("pis", "mus", "sigs")}   # (copies: the shared reference is read-only)


def _all_three(MD, samples, obs):
    m, _ = _mg()
    obs = np.array(obs)
    return (R.np_(MD.log_likelihood(m, samples, obs)["obs"]), R.np_(MD.log_predictive_density(m, samples, obs)),
            R.np_(MD.responsibilities(m, samples, obs)))


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("k,d,rows,n", ALL_CASES)
def test_outputs_inside_the_intervals(MD, k, d, rows, n, kind):
    """ll, lppd and resp inside the float64 intervals at every shape of mixture_ref.SHAPES with n in 1, 2, 5, the row tile's edges
    and the draw split's edges (four waves: n = 3, 5, 9; two waves at the largest shapes: n = 1, 3, 5)."""
    ref = D.reference(kind, k, d, rows, n)
    ll, lppd, resp = _all_three(MD, _samples(ref), ref["obs"])
    assert ll.shape == (n, rows) and lppd.shape == (rows,) and resp.shape == (rows, k)
    assert ll.dtype == lppd.dtype == resp.dtype == np.float32
    what = f"{kind} k={k} d={d} rows={rows} n={n}"
    D.inside(ll, ref["ll_lo"], ref["ll_hi"], what + " ll")
    D.inside(lppd, ref["lppd_lo"], ref["lppd_hi"], what + " lppd")
    D.inside(resp, ref["resp_lo"], ref["resp_hi"], what + " resp")
    assert np.all(np.abs(resp.astype(np.float64).sum(axis=1) - 1.0) <= k * (D.RESP_SLACK + 2.0 ** -24))


@pytest.mark.parametrize("n", [1, DT + 1, 2 * DT + 3])
def test_rows_form_against_the_reduced_form(MD, n):
    """The device's own (n, rows) reduced in float64 on the host: the reduced form's lppd lies within the reduction's slack of it
    (both forms compute ll with the same code, so nothing of a's bound enters)."""
    ref = D.reference("soft", 3, 5, T + 1, n)
    ll, lppd, _ = _all_three(MD, _samples(ref), ref["obs"])
    want = D.lse(ll.astype(np.float64), 0) - np.log(float(n))
    err = np.abs(lppd.astype(np.float64) - want)
    print(f"n={n}: max err / slack {np.max(err / D.slack(want)):.3f}")
    assert np.all(err <= D.slack(want))


@pytest.mark.parametrize("k,d,rows", R.SHAPES)
def test_one_draw_against_assignment_log_posterior(MD, k, d, rows):
    """n = 1: ll is the logsumexp of mixture.assignment_log_posterior's row on the same parameters, within the two kernels' bounds
    (logsumexp is 1-Lipschitz in the maximum norm) and the slack."""
    from d3p_amd import mixture as MX
    ref = D.reference("soft", k, d, rows, 1)
    m, _ = _mg()
    obs, one = np.array(ref["obs"]), _samples(ref)
    ll = R.np_(MD.log_likelihood(m, one, obs)["obs"])[0]
    a = R.np_(MX.assignment_log_posterior(obs, one["mus"][0], one["sigs"][0], one["pis"][0])).astype(np.float64)
    _, scale = R.a64(ref["obs"], ref["mus"][0], ref["sigs"][0], ref["pis"][0])
    want = R.logsumexp64(a)
    tol = (R.a_bound(scale) + D.bound(scale)).max(axis=1) + D.slack(want)
    err = np.abs(ll.astype(np.float64) - want)
    print(f"k={k} d={d} rows={rows}: max err / tol {np.max(err / tol):.3f}")
    assert np.all(err <= tol)


def _posterior_case(k=3, d=2, rows=T + 5, n=6):
    obs = D.soft_inputs(k, d, rows, 1)[0]
    return obs, R.posterior_params(k, d, 5), (k, obs, rows, d), n


def test_posterior_functions_equal_the_explicit_path_bit_for_bit(MD):
    """posterior_* draws the latents posterior_predictive_samples returns for the same key and reads them as that function's views
    are read: in place (no packing copy), with identical bits in every output."""
    from d3p_amd import mixture as MX
    m, g = _mg()
    obs, params, args, n = _posterior_case()
    key = R.key(31)
    samples = MX.posterior_predictive_samples(key, n, m, args, g, params)
    k, d = 3, 2
    with torch.cuda.device(samples["pis"].device):
        latent, ld = MD._pack(samples, n, k, d)
    assert latent.data_ptr() == samples["pis"].data_ptr() and ld == k + 2 * k * d          # read in place
    lppd = MD.log_predictive_density(m, samples, obs)
    resp = MD.responsibilities(m, samples, obs)
    got_lppd = MD.posterior_log_predictive_density(key, n, m, args, g, params)
    got_resp = MD.posterior_responsibilities(key, n, m, args, g, params)
    assert torch.equal(got_lppd, lppd) and torch.equal(got_resp, resp)
    both = MD.posterior_summary(key, n, m, args, g, params)
    assert sorted(both) == ["log_predictive_density", "responsibilities"]
    assert torch.equal(both["log_predictive_density"], lppd) and torch.equal(both["responsibilities"], resp)
    # obs= as a keyword, and another key gives other draws
    kw = MD.posterior_log_predictive_density(key, n, m, (k, None), g, params, obs=obs)
    assert torch.equal(kw, lppd)
    assert not torch.equal(MD.posterior_log_predictive_density(R.key(32), n, m, args, g, params), lppd)
    # a copy that is no packed view is packed once and gives the same bits
    copies = {name: v.clone() for name, v in samples.items() if name != "obs"}
    with torch.cuda.device(samples["pis"].device):
        packed, _ = MD._pack(copies, n, k, d)
    assert packed.data_ptr() not in (copies["pis"].data_ptr(), samples["pis"].data_ptr())
    assert torch.equal(MD.log_predictive_density(m, copies, obs), lppd)
    # sigs broadcast from (n, k, 1)
    flat = dict(copies, sigs=copies["sigs"][:, :, :1])
    wide = dict(copies, sigs=copies["sigs"][:, :, :1].expand(n, k, d).contiguous())
    assert torch.equal(MD.responsibilities(m, flat, obs), MD.responsibilities(m, wide, obs))


@pytest.mark.parametrize("k,d,rows,n", [(3, 2, 2 * T + 1, 2 * DT + 1), (16, 256, 5, 5)])
def test_two_calls_give_identical_bits(MD, k, d, rows, n):
    ref = D.reference("soft", k, d, rows, n)
    first = _all_three(MD, _samples(ref), ref["obs"])
    second = _all_three(MD, _samples(ref), ref["obs"])
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_special_values(MD):
    m, _ = _mg()
    obs, pis, mus, sigs = (np.array(v) for v in D.soft_inputs(3, 2, T + 3, 6))
    n, rows, k = 6, T + 3, 3
    base = _all_three(MD, {"pis": pis, "mus": mus, "sigs": sigs}, obs)
    # a zero weight: the component adds nothing and its responsibility in that draw is 0
    p0 = pis.copy()
    p0[:, 1] = 0.0
    ll, lppd, resp = _all_three(MD, {"pis": p0, "mus": mus, "sigs": sigs}, obs)
    assert np.isfinite(ll).all() and np.isfinite(lppd).all() and np.all(resp[:, 1] == 0.0)
    two = D.intervals(obs, np.delete(p0, 1, axis=1), np.delete(mus, 1, axis=1), np.delete(sigs, 1, axis=1))
    D.inside(ll, two["ll_lo"], two["ll_hi"], "zero weight ll")
    D.inside(resp[:, [0, 2]], two["resp_lo"], two["resp_hi"], "zero weight resp")
    # one draw with every component -inf: ll = -inf there, not NaN; lppd stays finite; that draw makes resp NaN (0 / 0)
    p1 = pis.copy()
    p1[2] = 0.0
    ll, lppd, resp = _all_three(MD, {"pis": p1, "mus": mus, "sigs": sigs}, obs)
    assert np.all(ll[2] == -np.inf) and np.array_equal(np.delete(ll, 2, axis=0), np.delete(base[0], 2, axis=0))
    five = D.intervals(obs, np.delete(pis, 2, axis=0), np.delete(mus, 2, axis=0), np.delete(sigs, 2, axis=0))
    shift = np.log(5.0) - np.log(6.0)   # the dead draw adds nothing to the sum and counts in n
    D.inside(lppd, five["lppd_lo"] + shift, five["lppd_hi"] + shift, "dead draw lppd")
    assert np.isnan(resp).all()
    # every draw -inf: lppd = -inf
    ll, lppd, resp = _all_three(MD, {"pis": np.zeros_like(pis), "mus": mus, "sigs": sigs}, obs)
    assert np.all(ll == -np.inf) and np.all(lppd == -np.inf) and np.isnan(resp).all()
    # NaN in one row of obs: that row's outputs are NaN, every other row is untouched
    x = obs.copy()
    x[T + 1, 1] = np.nan
    ll, lppd, resp = _all_three(MD, {"pis": pis, "mus": mus, "sigs": sigs}, x)
    assert np.isnan(ll[:, T + 1]).all() and np.isnan(lppd[T + 1]) and np.isnan(resp[T + 1]).all()
    keep = np.arange(rows) != T + 1
    assert np.array_equal(ll[:, keep], base[0][:, keep]) and np.array_equal(lppd[keep], base[1][keep]) and np.array_equal(resp[keep], base[2][keep])
    # NaN in one draw's latents (one component's mean; one scale; one weight): that draw's ll is NaN for every row, and the
    # reduced outputs with it; the other draws' ll are untouched
    for site, index in (("mus", (4, 2, 0)), ("sigs", (4, 0, 1)), ("pis", (4, 1))):
        bad = {"pis": pis.copy(), "mus": mus.copy(), "sigs": sigs.copy()}
        bad[site][index] = np.nan
        ll, lppd, resp = _all_three(MD, bad, obs)
        assert np.isnan(ll[4]).all(), site
        assert np.array_equal(np.delete(ll, 4, axis=0), np.delete(base[0], 4, axis=0)), site
        assert np.isnan(lppd).all() and np.isnan(resp).all(), site


CANARY = 0x7FC0DEAD


def _guarded(count, dtype, pad=64):
    whole = torch.full((count + 2 * pad,), CANARY, dtype=torch.int32, device="cuda")
    return whole, whole[pad:pad + count].view(dtype), pad


@pytest.mark.parametrize("k,d,rows,n", [(3, 2, T + 1, DT + 1), (16, 256, 5, 3), (5, 3, 2 * T - 1, 2)])
def test_canaries_around_every_output(MD, gpu, k, d, rows, n):
    import d3p_amd._lib as L
    from d3p_amd._lib import check, ptr, stream_ptr
    lib = L.load()
    ref_in = D.soft_inputs(k, d, rows, n)
    x = torch.tensor(ref_in[0]).cuda()
    ld = k + 2 * k * d + 3   # (a leading dimension above the row's length)
    lat = torch.zeros((n, ld), device="cuda")
    lat[:, :k], lat[:, k:k + k * d], lat[:, k + k * d:k + 2 * k * d] = (torch.tensor(ref_in[1]).cuda(), torch.tensor(ref_in[2]).cuda().reshape(n, -1),
                                                                        torch.tensor(ref_in[3]).cuda().reshape(n, -1))
    bufs = {"ll": _guarded(n * rows, torch.float32), "lppd": _guarded(rows, torch.float32), "resp": _guarded(rows * k, torch.float32),
            "lppd_alone": _guarded(rows, torch.float32), "resp_alone": _guarded(rows * k, torch.float32)}
    v = {name: b[1] for name, b in bufs.items()}
    check(lib.d3p_gmm_loglik_rows(stream_ptr(), ptr(x), rows, d, ptr(lat), ld, k, n, ptr(v["ll"])))
    check(lib.d3p_gmm_loglik_reduce(stream_ptr(), ptr(x), rows, d, ptr(lat), ld, k, n, ptr(v["lppd"]), ptr(v["resp"])))
    check(lib.d3p_gmm_loglik_reduce(stream_ptr(), ptr(x), rows, d, ptr(lat), ld, k, n, ptr(v["lppd_alone"]), None))
    check(lib.d3p_gmm_loglik_reduce(stream_ptr(), ptr(x), rows, d, ptr(lat), ld, k, n, None, ptr(v["resp_alone"])))
    torch.cuda.synchronize()
    for name, (whole, view, pad) in bufs.items():
        w = R.np_(whole)
        assert np.all(w[:pad] == CANARY) and np.all(w[pad + view.numel():] == CANARY), name
        assert not np.any(R.np_(view.view(torch.int32)) == CANARY), name   # every element was written
    assert torch.equal(v["lppd"], v["lppd_alone"]) and torch.equal(v["resp"], v["resp_alone"])
    m, _ = _mg()
    samples = {"pis": ref_in[1], "mus": ref_in[2], "sigs": ref_in[3]}
    assert torch.equal(MD.log_likelihood(m, samples, ref_in[0])["obs"].reshape(-1), v["ll"])
    assert torch.equal(MD.responsibilities(m, samples, ref_in[0]).reshape(-1), v["resp"])


def test_views_of_obs(MD):
    """Non-contiguous and offset views of obs give the bits of the contiguous copy."""
    m, _ = _mg()
    obs, pis, mus, sigs = D.soft_inputs(3, 5, T + 2, 3)
    samples = {"pis": pis, "mus": mus, "sigs": sigs}
    want = MD.responsibilities(m, samples, obs), MD.log_predictive_density(m, samples, obs)
    big = torch.full((2 * (T + 2) + 1, 9), 7.0, device="cuda")
    big[1::2, 3:8] = torch.tensor(obs).cuda()
    for view in (big[1::2, 3:8], big[1::2, 3:8].t().contiguous().t(), torch.tensor(obs).cuda()[:, :]):
        assert torch.equal(MD.responsibilities(m, samples, view), want[0]) and torch.equal(MD.log_predictive_density(m, samples, view), want[1])
    assert torch.equal(big[0], torch.full((9,), 7.0, device="cuda"))   # (nothing written into the view's parent)
    off = torch.zeros((T + 2) * 5 + 1, device="cuda")
    off[1:] = torch.tensor(obs).cuda().reshape(-1)
    assert torch.equal(MD.responsibilities(m, samples, off[1:].view(T + 2, 5)), want[0])


def test_zero_rows(MD, gpu):
    import d3p_amd._lib as L
    from d3p_amd._lib import ptr, stream_ptr
    m, _ = _mg()
    _, pis, mus, sigs = D.soft_inputs(3, 2, 4, 2)
    samples = {"pis": pis, "mus": mus, "sigs": sigs}
    empty = np.zeros((0, 2), np.float32)
    assert tuple(MD.log_likelihood(m, samples, empty)["obs"].shape) == (2, 0)
    assert tuple(MD.log_predictive_density(m, samples, empty).shape) == (0,)
    assert tuple(MD.responsibilities(m, samples, empty).shape) == (0, 3)
    one = torch.zeros(1, device="cuda")
    lib = L.load()
    assert lib.d3p_gmm_loglik_rows(stream_ptr(), ptr(one), 0, 2, ptr(one), 15, 3, 2, ptr(one)) == 0
    assert lib.d3p_gmm_loglik_reduce(stream_ptr(), ptr(one), 0, 2, ptr(one), 15, 3, 2, ptr(one), ptr(one)) == 0
    torch.cuda.synchronize()
    assert float(one[0]) == 0.0


def test_c_entries_refuse_before_any_launch(gpu):
    import d3p_amd._lib as L
    from d3p_amd._lib import ptr, stream_ptr
    lib = L.load()
    one = torch.zeros(1, device="cuda")
    p = ptr(one)
    UNSUPPORTED, INVALID = -3, -1

    def rows_(k, d, rows, n=1, x=p, lat=p, out=p, ld=None):
        return lib.d3p_gmm_loglik_rows(stream_ptr(), x, rows, d, lat, k + 2 * k * d if ld is None else ld, k, n, out)

    def reduce_(k, d, rows, n=1, x=p, lat=p, lppd=p, resp=p, ld=None):
        return lib.d3p_gmm_loglik_reduce(stream_ptr(), x, rows, d, lat, k + 2 * k * d if ld is None else ld, k, n, lppd, resp)

    for k, d in ((17, 256), (33, 1), (32, 129), (1, 257)):
        assert rows_(k, d, 4) == UNSUPPORTED and reduce_(k, d, 4) == UNSUPPORTED, (k, d)
    for k, d in ((0, 2), (2, 0)):
        assert rows_(k, d, 4) == INVALID and reduce_(k, d, 4) == INVALID, (k, d)
    assert rows_(1, 1, 2 ** 32) == UNSUPPORTED and rows_(2, 256, 2 ** 24) == UNSUPPORTED and reduce_(2, 256, 2 ** 24) == UNSUPPORTED
    assert b"2^32" in lib.d3p_last_error()
    assert rows_(3, 2, 4, n=0) == INVALID and reduce_(3, 2, 4, n=0) == INVALID
    assert rows_(3, 2, 4, n=2 ** 31) == UNSUPPORTED and reduce_(3, 2, 4, n=2 ** 31) == UNSUPPORTED
    assert rows_(3, 2, 4, ld=14) == INVALID and reduce_(3, 2, 4, ld=14) == INVALID           # a latent row holds k + 2 k d = 15 values
    assert rows_(3, 2, 4, x=None) == INVALID and rows_(3, 2, 4, lat=None) == INVALID and rows_(3, 2, 4, out=None) == INVALID
    assert reduce_(3, 2, 4, x=None) == INVALID and reduce_(3, 2, 4, lat=None) == INVALID
    assert reduce_(3, 2, 4, lppd=None, resp=None) == INVALID                                   # neither output
    assert b"at least one" in lib.d3p_last_error()
    odd = C.c_void_p(one.data_ptr() + 2)
    assert rows_(3, 2, 4, out=odd) == INVALID and reduce_(3, 2, 4, x=odd) == INVALID and reduce_(3, 2, 4, resp=odd) == INVALID
    assert b"aligned" in lib.d3p_last_error()
    host = np.zeros(64, np.float32)
    hp = C.c_void_p(host.ctypes.data)
    assert rows_(3, 2, 4, x=hp) == INVALID and reduce_(3, 2, 4, lat=hp) == INVALID and reduce_(3, 2, 4, lppd=hp) == INVALID
    assert b"device memory" in lib.d3p_last_error()
    assert rows_(3, 2, 0) == 0 and reduce_(3, 2, 0) == 0                                       # rows == 0: D3P_OK, no launch
    torch.cuda.synchronize()
    assert float(one[0]) == 0.0


def test_example_reports_held_out_density_behind_its_flag(MD, capsys):
    spec = importlib.util.spec_from_file_location("ex_gmm_density", os.path.join(ROOT, "examples", "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args([]).held_out_density is False                       # off by default
    args = mod.parse_args("--sigma 1.0 -N 512 -n 2 --held-out-density --posterior-draws 7".split())
    acc, pis, modes = mod.main(args)
    out = capsys.readouterr().out
    lppd = re.search(r"held-out log predictive density \(mean over 512 points, 7 posterior draws\): (-?[\d.]+)", out)
    soft = re.search(r"assignment accuracy \(argmax of posterior responsibilities\): ([\d.]+)", out)
    assert lppd and soft and "assignment accuracy: " in out
    assert np.isfinite(float(lppd.group(1))) and 0.0 <= float(soft.group(1)) <= 1.0
    # the same figures from the module, on the parameters main returned (mean of Dirichlet(alpha) -> alpha up to a factor is not
    # recoverable, so only the call's shape is checked here)
    X_train, X_test, z_test, true_mus = mod.create_toy_data(512, 2)
    params = {"alpha_log": torch.zeros(3, device="cuda"), "mus_loc": modes}
    value, soft_acc = mod.held_out_density(X_test, z_test, params, 3, 7)
    assert np.isfinite(value) and 0.0 <= soft_acc <= 1.0
