"""d3p_amd.mixture on the GPU against tests/mixture_ref.py (tolerances and the calibrated assignment bound are stated there): prior
and posterior predictive draws at every tile edge of k_predict_gmm_obs, the component rule's special cases, the product-then-sum
rule bit for bit, the key rule, canaries around every output, assignment_log_posterior / assign, the C entries' refusals and the
example's opt-in flags."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from . import mixture_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = R.T


@pytest.fixture(scope="module")
def MX(gpu):
    from d3p_amd import mixture
    return mixture


def _mg():
    from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel
    m = GaussianMixtureModel()
    return m, GaussianMixtureGuide(m)


def _host(res, multi):
    """The device's dict (with intermediates) as numpy arrays with a leading draw axis; zs under 'zs'."""
    out = {}
    for name, (v, inter) in res.items():
        out[name] = R.np_(v) if multi else R.np_(v)[None]
        if name == "obs":
            assert isinstance(inter, tuple) and len(inter) == 1
            out["zs"] = R.np_(inter[0]) if multi else R.np_(inter[0])[None]
        else:
            assert len(inter) == 0
    return out


def _check_draws(O, res, exp, k, d, rows, subst, what):
    n = len(exp)
    assert res["pis"].shape == (n, k) and res["mus"].shape == (n, k, d) and res["sigs"].shape == (n, k, d)
    assert res["obs"].shape == (n, rows, d) and res["zs"].shape == (n, rows) and res["obs"].dtype == np.float32
    R.check_latents(res, exp, k, d, subst, what)
    for i, e in enumerate(exp):
        R.check_obs(O, res["pis"][i], res["mus"][i], res["sigs"][i], res["obs"][i], res["zs"][i], e["obs_key"], f"{what} draw {i}")


@pytest.mark.parametrize("posterior", [False, True], ids=["prior", "posterior"])
@pytest.mark.parametrize("k,d,rows", R.DRAW_SHAPES)
def test_draws_vs_oracle(MX, O, k, d, rows, posterior):
    """n in 1, 2, 3 and the single form (checked against the oracle on rng_key itself) at every shape: one row, odd rows d (the
    half-offset pairing of the normals), the row tile's edges and the largest k and d."""
    m, g = _mg()
    params = R.posterior_params(k, d, 5) if posterior else None
    seed = 100 * k + rows
    for n in (None, 1, 2, 3):
        multi = n is not None
        if posterior:
            res = MX.posterior_predictive_samples(R.key(seed), n, m, (k, None, rows, d), g, params, with_intermediates=True)
        else:
            res = MX.prior_predictive_samples(R.key(seed), n, m, (k, None, rows, d), with_intermediates=True)
        exp = R.expect_latents(O, R.key_words(seed), n or 1, multi, k, d, params)
        _check_draws(O, _host(res, multi), exp, k, d, rows, {}, f"k={k} d={d} rows={rows} n={n}")
    plain = MX.prior_predictive_samples(R.key(seed), None, m, (k, None, rows, d))
    assert set(plain) == {"pis", "mus", "sigs", "obs"} and tuple(plain["obs"].shape) == (rows, d) and plain["obs"].is_cuda


def _fixed(MX, seed, pis, rows, d=1, mus=None, sigs=None, n=None):
    k = len(pis)
    m, _ = _mg()
    sub = {"pis": np.asarray(pis, np.float32), "mus": np.zeros((k, d), np.float32) if mus is None else mus,
           "sigs": np.ones((k, d), np.float32) if sigs is None else sigs}
    res = MX.prior_predictive_samples(R.key(seed), n, m, (k, None, rows, d), substitutes=sub, with_intermediates=True)
    return R.np_(res["obs"][0]), R.np_(res["obs"][1][0]), sub


def test_component_rule_special_cases(MX, O):
    _, zs, _ = _fixed(MX, 3, (1, 0, 0), 1000)
    assert np.all(zs == 0)
    _, zs, _ = _fixed(MX, 3, (0, 0, 1), 1000)
    assert np.all(zs == 2)
    # 31 x float32(1/31): the float32 running sum ends at 1 - 2^-21; key 29 (found by searching on the CPU with the oracle) has a
    # uniform above it at row 53652, whose count reaches k and is clamped to k - 1
    pis = np.full(31, 1.0 / 31, np.float32)
    top = np.cumsum(pis, dtype=np.float32)[-1]
    rows = 1 << 16
    sk = R.site_keys(O, R.key_words(29), False, ("pis", "mus", "sigs"))
    u = O.tf_uniform(O.tf_split(sk["obs"], 2)[0], rows)
    assert top < 1 and u[53652] > top
    _, zs, _ = _fixed(MX, 29, pis, rows)
    assert zs[53652] == 30 and np.array_equal(zs, R.component_rule(pis, u))
    # frequencies at (1/4, 1/4, 1/2) over 2^16 rows within 5 standard deviations
    p = np.array([0.25, 0.25, 0.5])
    _, zs, _ = _fixed(MX, 7, p, rows)
    cnt = np.bincount(zs, minlength=3)
    assert cnt.sum() == rows and np.all(np.abs(cnt - rows * p) <= 5 * np.sqrt(rows * p * (1 - p))), cnt


def test_product_then_sum_bit_for_bit(MX):
    """With mus = 0 and sigs = 1 substituted the outcomes are the device's eps; with general mus and sigs and the same key they must
    be fl(mus[z] + fl(sigs[z] eps)) in numpy float32, bit for bit (a contraction into one fma would show here)."""
    k, d, rows = 3, 5, T + 1
    pis = (0.25, 0.25, 0.5)
    eps, z0, _ = _fixed(MX, 11, pis, rows, d)
    r = np.random.default_rng(4)
    mus = (3 * r.normal(size=(k, d))).astype(np.float32)
    sigs = r.uniform(0.05, 3.0, (k, d)).astype(np.float32)
    xs, z, _ = _fixed(MX, 11, pis, rows, d, mus, sigs)
    assert np.array_equal(z, z0) and len(set(z.tolist())) == 3
    want = mus[z] + sigs[z] * eps
    assert want.dtype == np.float32 and np.array_equal(xs.view(np.uint32), want.view(np.uint32))
    fused = (mus[z].astype(np.float64) + sigs[z].astype(np.float64) * eps.astype(np.float64)).astype(np.float32)
    assert not np.array_equal(fused, want)   # (the two forms do differ on these inputs: the check can tell them apart)


def test_key_rule(MX, O):
    """A substituted site takes no key, so the later sites' keys shift; prior and posterior differ at the same key."""
    k, d, rows = 3, 2, 9
    m, g = _mg()
    mus = np.arange(6, dtype=np.float32).reshape(k, d)
    with_sub = _host(MX.prior_predictive_samples(R.key(5), 2, m, (k, None, rows, d), substitutes={"mus": mus}, with_intermediates=True), True)
    without = _host(MX.prior_predictive_samples(R.key(5), 2, m, (k, None, rows, d), with_intermediates=True), True)
    _check_draws(O, with_sub, R.expect_latents(O, R.key_words(5), 2, True, k, d, subst={"mus": mus}), k, d, rows, {"mus": mus}, "mus given")
    _check_draws(O, without, R.expect_latents(O, R.key_words(5), 2, True, k, d), k, d, rows, {}, "nothing given")
    assert np.array_equal(with_sub["pis"], without["pis"]) and not np.array_equal(with_sub["sigs"], without["sigs"])
    # sigs broadcast from (k, 1), as the reference's example passes them
    sg = np.array([[0.1], [1.0], [0.1]], np.float32)
    res = _host(MX.prior_predictive_samples(R.key(5), 2, m, (k, None, rows, d), substitutes={"sigs": sg}, with_intermediates=True), True)
    _check_draws(O, res, R.expect_latents(O, R.key_words(5), 2, True, k, d, subst={"sigs": sg}), k, d, rows, {"sigs": sg}, "sigs given")
    params = {"alpha_log": np.zeros(k, np.float32), "mus_loc": np.zeros((k, d), np.float32)}
    post = _host(MX.posterior_predictive_samples(R.key(5), 2, m, (k, None, rows, d), g, params, with_intermediates=True), True)
    assert not np.array_equal(post["pis"], without["pis"]) and not np.array_equal(post["obs"], without["obs"])
    # obs given: only its shape is used
    again = _host(MX.prior_predictive_samples(R.key(5), 2, m, (k, torch.zeros(rows, d)), with_intermediates=True), True)
    assert np.array_equal(again["obs"], without["obs"])


def test_two_calls_give_identical_bits(MX):
    m, g = _mg()
    params = R.posterior_params(16, 64, 1)
    a = MX.posterior_predictive_samples(R.key(9), 3, m, (16, None, 300, 64), g, params, with_intermediates=True)
    b = MX.posterior_predictive_samples(R.key(9), 3, m, (16, None, 300, 64), g, params, with_intermediates=True)
    for name in a:
        assert torch.equal(a[name][0], b[name][0]), name
    assert torch.equal(a["obs"][1][0], b["obs"][1][0])


CANARY = 0x7FC0DEAD


def _guarded(count, dtype, pad=64):
    """(whole buffer as int32 words filled with the canary, the view of `count` elements in its middle)."""
    whole = torch.full((count + 2 * pad,), CANARY, dtype=torch.int32, device="cuda")
    return whole, whole[pad:pad + count].view(dtype), pad


def _intact(whole, count, pad):
    w = R.np_(whole)
    return np.all(w[:pad] == CANARY) and np.all(w[pad + count:] == CANARY)


def test_canaries_around_every_output(MX, gpu):
    import d3p_amd._lib as L
    from d3p_amd._lib import check, ptr, stream_ptr
    lib = L.load()
    k, d, rows, n = 3, 2, T + 1, 2
    kd = k * d
    bufs = {"latent": _guarded(n * (k + 2 * kd), torch.float32), "keys": _guarded(2 * n, torch.int32),
            "obs": _guarded(n * rows * d, torch.float32), "zs": _guarded(n * rows, torch.int32),
            "a": _guarded(rows * k, torch.float32), "arg": _guarded(rows, torch.int32)}
    v = {name: b[1] for name, b in bufs.items()}
    check(lib.d3p_predict_gmm_draws(stream_ptr(), ptr(R.key(2)), n, 1, 0, k, d, None, None, 10.0, None, None, None, ptr(v["latent"]),
                                    ptr(v["keys"])))
    check(lib.d3p_predict_gmm_obs(stream_ptr(), ptr(v["latent"]), k + 2 * kd, k, d, rows, n, ptr(v["keys"]), ptr(v["obs"]), ptr(v["zs"])))
    lat = v["latent"].view(n, k + 2 * kd)
    check(lib.d3p_gmm_assign(stream_ptr(), ptr(v["obs"]), rows, d, ptr(lat[0, k:k + kd]), ptr(lat[0, k + kd:]), ptr(lat[0, :k]), k,
                             ptr(v["a"]), ptr(v["arg"])))
    torch.cuda.synchronize()
    for name, (whole, view, pad) in bufs.items():
        assert _intact(whole, view.numel(), pad), name
        assert not np.any(R.np_(view.view(torch.int32)) == CANARY), name   # every element was written
    m, _ = _mg()
    same = MX.prior_predictive_samples(R.key(2), n, m, (k, None, rows, d), with_intermediates=True)
    assert torch.equal(same["obs"][0].reshape(-1), v["obs"]) and torch.equal(same["obs"][1][0].reshape(-1), v["zs"])


@pytest.mark.parametrize("k,d,rows", R.SHAPES)
def test_assignment_vs_float64(MX, k, d, rows):
    obs, mus, sigs, pis = R.assign_inputs(k, d, rows)
    a = R.np_(MX.assignment_log_posterior(obs, mus, sigs, pis))
    arg = R.np_(MX.assign(torch.tensor(obs).cuda(), mus, sigs, pis))
    assert a.shape == (rows, k) and a.dtype == np.float32 and arg.shape == (rows,) and arg.dtype == np.int32
    ref, scale = R.a64(obs, mus, sigs, pis)
    bound = R.a_bound(scale)
    err = np.abs(a.astype(np.float64) - ref)
    print(f"k={k} d={d} rows={rows}: max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), np.max(err / bound)
    # logsumexp is 1-Lipschitz in the maximum norm: the row's log_prob lies within the row's largest bound
    assert np.all(np.abs(R.logsumexp64(a.astype(np.float64)) - R.logsumexp64(ref)) <= bound.max(axis=1))
    judged = R.judged_rows(ref, bound)
    assert np.array_equal(arg[judged], ref.argmax(axis=1)[judged])
    assert np.all((arg >= 0) & (arg < k))
    R.assert_not_vacuous(1.0 - judged.mean(), rows, f"k={k} d={d} rows={rows}")


def test_assignment_ties_nan_and_single_outputs(MX, gpu):
    import d3p_amd._lib as L
    from d3p_amd._lib import check, ptr, stream_ptr
    obs, mus, sigs, pis = R.assign_inputs(3, 2, 40)
    mus[1], sigs[1], pis[:] = mus[0], sigs[0], (0.3, 0.3, 0.4)   # two identical components: the first wins
    z = np.arange(40) % 3
    obs = (mus[z] + 0.01).astype(np.float32)
    arg = R.np_(MX.assign(obs, mus, sigs, pis))
    assert np.array_equal(arg, np.where(z == 2, 2, 0))
    obs[5, 1] = np.nan
    a = R.np_(MX.assignment_log_posterior(obs, mus, sigs, pis))
    arg = R.np_(MX.assign(obs, mus, sigs, pis))
    assert np.isnan(a[5]).all() and arg[5] == -1 and not np.isnan(np.delete(a, 5, axis=0)).any() and np.all(np.delete(arg, 5) >= 0)
    sig_nan = sigs.copy()
    sig_nan[2, 0] = np.nan   # a NaN in one component only: the whole row of a is NaN all the same
    a2 = R.np_(MX.assignment_log_posterior(obs[:3], mus, sig_nan, pis))
    assert np.isnan(a2).all() and np.all(R.np_(MX.assign(obs[:3], mus, sig_nan, pis)) == -1)
    # both outputs in one call agree with the two single-output calls
    t = [torch.tensor(x).cuda() for x in (obs, mus, sigs, pis)]
    both_a = torch.empty((40, 3), device="cuda")
    both_arg = torch.empty(40, dtype=torch.int32, device="cuda")
    check(L.load().d3p_gmm_assign(stream_ptr(), ptr(t[0]), 40, 2, ptr(t[1]), ptr(t[2]), ptr(t[3]), 3, ptr(both_a), ptr(both_arg)))
    assert np.array_equal(R.np_(both_a), a, equal_nan=True) and np.array_equal(R.np_(both_arg), arg)
    assert tuple(MX.assign(np.zeros((0, 2), np.float32), mus, sigs, pis).shape) == (0,)


def test_c_entries_refuse_before_any_launch(gpu):
    import d3p_amd._lib as L
    from d3p_amd._lib import ptr, stream_ptr
    lib = L.load()
    one = torch.zeros(1, device="cuda")
    keys = torch.zeros(2, dtype=torch.int32, device="cuda")
    p, kp = ptr(one), ptr(keys)
    UNSUPPORTED, INVALID = -3, -1

    def draws(k, d, n=1):
        return lib.d3p_predict_gmm_draws(stream_ptr(), kp, n, 1, 0, k, d, None, None, 10.0, None, None, None, p, kp)

    def obs(k, d, rows, n=1, lat=p, out=p):
        return lib.d3p_predict_gmm_obs(stream_ptr(), lat, k + 2 * k * d, k, d, rows, n, kp, out, None)

    def assign(k, d, rows, x=p, a=p):
        return lib.d3p_gmm_assign(stream_ptr(), x, rows, d, p, p, p, k, a, None)

    for k, d in ((17, 256), (33, 1), (32, 129), (1, 257)):
        assert draws(k, d) == UNSUPPORTED and obs(k, d, 4) == UNSUPPORTED and assign(k, d, 4) == UNSUPPORTED, (k, d)
    for k, d in ((0, 2), (2, 0)):
        assert draws(k, d) == INVALID and obs(k, d, 4) == INVALID and assign(k, d, 4) == INVALID, (k, d)
    assert obs(1, 1, 2 ** 32) == UNSUPPORTED and obs(2, 256, 2 ** 24) == UNSUPPORTED and assign(2, 256, 2 ** 24) == UNSUPPORTED
    assert b"2^32" in lib.d3p_last_error()
    assert obs(3, 2, 0) == 0 and assign(3, 2, 0) == 0                       # rows == 0: D3P_OK, no launch
    assert draws(3, 2, 0) == INVALID and obs(3, 2, 4, n=0) == INVALID
    assert obs(3, 2, 4, lat=None) == INVALID and obs(3, 2, 4, out=None) == INVALID and assign(3, 2, 4, x=None) == INVALID
    assert assign(3, 2, 4, a=None) == INVALID                                # neither output
    odd = C.c_void_p(one.data_ptr() + 2)
    assert obs(3, 2, 4, out=odd) == INVALID and assign(3, 2, 4, x=odd) == INVALID
    assert b"aligned" in lib.d3p_last_error()
    torch.cuda.synchronize()
    assert float(one[0]) == 0.0


def test_example_with_predictive_toy_data_and_posterior_assignment(MX):
    spec = importlib.util.spec_from_file_location("ex_gmm_mixture", os.path.join(ROOT, "examples", "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    N, d = 512, 2
    X_train, X_test, z_test, true_mus = mod.create_toy_data_predictive(N, d)
    m, _ = _mg()
    mus = np.array([-10.0, 10.0, -2.0], np.float32)[:, None] * np.ones((1, d), np.float32)
    direct = MX.prior_predictive_samples(R.key(1234), None, m, (3, None, 2 * N, d), with_intermediates=True,
                                         substitutes={"pis": [0.25, 0.25, 0.5], "mus": mus, "sigs": np.array([[0.1], [1.0], [0.1]], np.float32)})
    assert torch.equal(torch.cat([X_train, X_test]), direct["obs"][0]) and torch.equal(z_test, direct["obs"][1][0][N:])
    args = mod.parse_args("--toy-data predictive --assignment posterior --sigma 1.0 -N 512 -n 2".split())
    assert (args.toy_data, args.assignment, args.num_samples, args.num_epochs, args.dimensions) == ("predictive", "posterior", N, 2, d)
    acc, pis, modes = mod.main(args)
    assert 0.0 <= acc <= 1.0 and tuple(modes.shape) == (3, d)
