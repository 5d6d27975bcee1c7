"""CPU comparator of d3p_amd.mixture for tests/test_mixture_host.py and tests/test_gpu_mixture.py.

Built from the oracle's threefry functions (tf_split, tf_uniform, tf_normal, tf_random_words, gamma_sample) and from
tests/predictive_ref.py's draw_keys / chains / site_key / assert_not_vacuous, following DESIGN.md section 4f.

Tolerances of the latents are those tests/test_gpu_gmm_model.py::test_px_grads_and_latents_vs_oracle uses for exactly these quantities:
  * pis   rtol 2e-6 (the gamma draws; float64 on both sides, log / pow differ in the last ulp)
  * mus   the normals at atol 1e-6, times the site's scale
  * sigs  rtol 2e-6 (logf differs in the last ulp)
obs is judged against the latents the DEVICE returned, so none of the above leaks into it:
  * zs    equal to min(#{j : cum_j < u}, k - 1) with cum = np.cumsum(float32) and the oracle's u: exact bits on both sides, no band
  * xs    within |sigs[z]| 1e-6 plus one float32 ulp of the result of mus[z] + sigs[z] eps with the oracle's eps

assignment_log_posterior: the float64 comparator `a64` against the device's float32 direct form.  The per-element bound is
    bound[r, j] = A_BOUND_ULPS 2^-24 scale[r, j],   scale[r, j] = sum_c (z^2 / 2 + |log sig| + log(2 pi) / 2) + |log pis_j|,
the sum of the magnitudes of the terms of a[r, j] (its condition scale).  Calibrated on the CPU (test_mixture_host.py::
test_assignment_bound_calibration) with a numpy float32 restatement of the direct form, summed over c in index order, over the GPU
tests' inputs (assign_inputs at every shape of SHAPES): the largest error seen is A_ERR_SEEN_ULPS = 11.11 in units of 2^-24 scale
(at k = 16, d = 256: a serial float32 sum of 256 terms); A_BOUND_ULPS = 4 x that = 44.44.  The factor covers logf and the division differing in the last ulp between libm and the device and
the order of the cross-lane sum (the same reason the project's link_tols carry a margin).
"""
import numpy as np

from d3p_amd import mixture as MX
from .predictive_ref import assert_not_vacuous, chains, draw_keys, key, key_words, np_, site_key  # noqa: F401

T = MX.ROW_TILE
# the shapes the checks are set for; DRAW_SHAPES adds one with several workgroups, several passes of the pair loop and a column carry
# (5 does not divide 256), so that the upper range of a later workgroup is judged against the oracle too
SHAPES = [(1, 1, 1), (2, 1, 2), (3, 5, 3), (3, 2, T - 1), (3, 2, T), (3, 2, T + 1), (16, 256, 5), (32, 128, 5)]   # (k, d, rows)

DRAW_SHAPES = SHAPES + [(3, 5, 2 * T + 1)]

A_ERR_SEEN_ULPS = 11.11
A_BOUND_ULPS = 44.44
HALF_LOG_2PI = 0.918938533204672742


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def sigs_rule(words):
    """1 / -logf(u), u = ((bits >> 9) + 0.5) 2^-23, in numpy float32."""
    u = ((words >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    return (np.float32(1.0) / -np.log(u)).astype(np.float32)


def site_keys(O, dk, posterior, substituted=()):
    """{site: its threefry key or None} of one draw with key `dk`, by mixture._key_plan."""
    mk, gk = chains(O, dk, posterior)
    return {st.name: (None if st.key_index is None else site_key(O, gk if st.chain == "guide" else mk, st.key_index))
            for st in MX._key_plan(posterior, substituted)}


def expect_latents(O, rng_key, n, multi, k, d, params=None, subst=None, prior_mu_scale=10.0):
    """Per draw: {"pis": float64 (k,) or given, "mus": (loc, eps, scale) or given, "sigs": float32 (k d) or given, "obs_key"}."""
    posterior = params is not None
    subst = subst or {}
    out = []
    for dk in draw_keys(O, rng_key, n, multi):
        sk = site_keys(O, dk, posterior, set(subst))
        e = {"obs_key": sk["obs"]}
        if sk["pis"] is None:
            e["pis"] = np.asarray(subst["pis"], np.float32)
        else:
            alpha = np.exp(params["alpha_log"].astype(np.float64)) if posterior else np.ones(k)
            g = np.array([O.gamma_sample(sk["pis"], j, float(alpha[j])) for j in range(k)])
            S = 0.0
            for v in g:
                S += v
            e["pis"] = g / S
        if sk["mus"] is None:
            e["mus"] = np.broadcast_to(np.asarray(subst["mus"], np.float32), (k, d))
        else:
            loc = params["mus_loc"].astype(np.float64).ravel() if posterior else np.zeros(k * d)
            e["mus"] = (loc, O.tf_normal(sk["mus"], k * d), 1.0 if posterior else float(prior_mu_scale))
        if sk["sigs"] is None:
            e["sigs"] = np.broadcast_to(np.asarray(subst["sigs"], np.float32), (k, d))
        else:
            e["sigs"] = sigs_rule(O.tf_random_words(sk["sigs"], k * d))
        out.append(e)
    return out


def check_latents(res, exp, k, d, subst, what):
    """res: the device's dict with a leading n axis (numpy)."""
    for i, e in enumerate(exp):
        if "pis" in subst:
            assert np.array_equal(res["pis"][i], e["pis"]), f"{what}: substituted pis"
        else:
            np.testing.assert_allclose(res["pis"][i], e["pis"], rtol=2e-6, err_msg=f"{what} pis[{i}]")
        if "mus" in subst:
            assert np.array_equal(res["mus"][i], e["mus"]), f"{what}: substituted mus"
        else:
            loc, eps, scale = e["mus"]
            ref = loc + eps.astype(np.float64) * scale
            err = np.abs(res["mus"][i].ravel().astype(np.float64) - ref)
            print(f"{what} mus[{i}]: max err {err.max():.3e} of {1e-6 * scale:.1e}")
            assert np.all(err <= 1e-6 * scale), f"{what} mus[{i}]: max err {err.max()}"
        if "sigs" in subst:
            assert np.array_equal(res["sigs"][i], e["sigs"]), f"{what}: substituted sigs"
        else:
            np.testing.assert_allclose(res["sigs"][i].ravel(), e["sigs"], rtol=2e-6, err_msg=f"{what} sigs[{i}]")


def component_rule(pis32, u):
    """z = min(#{j : cum_j < u}, k - 1), cum the float32 running sum left to right (np.cumsum)."""
    cum = np.cumsum(np.asarray(pis32, np.float32), dtype=np.float32)
    return np.minimum((cum[None, :] < np.asarray(u, np.float32)[:, None]).sum(axis=1), len(cum) - 1).astype(np.int32)


def obs_streams(O, obs_key, rows, d):
    """(u (rows,), eps (rows, d)) of GaussianMixture.sample_with_intermediates on the oracle."""
    ks = O.tf_split(obs_key, 2)
    return O.tf_uniform(ks[0], rows), O.tf_normal(ks[1], rows * d).reshape(rows, d)


def check_obs(O, pis, mus, sigs, xs, zs, obs_key, what):
    """One draw's outcomes against the device's own latents (numpy float32: pis (k,), mus / sigs (k, d), xs (rows, d), zs (rows,))."""
    rows, d = xs.shape
    u, eps = obs_streams(O, obs_key, rows, d)
    z = component_rule(pis, u)
    assert zs.dtype == np.int32 and np.array_equal(zs, z), f"{what}: zs differ at rows {np.flatnonzero(zs != z)[:8]}"
    ref = mus[z].astype(np.float64) + sigs[z].astype(np.float64) * eps.astype(np.float64)
    err = np.abs(xs.astype(np.float64) - ref)
    tol = np.abs(sigs[z].astype(np.float64)) * 1e-6 + ulp32(ref)
    assert np.all(err <= tol), f"{what}: xs max err {err.max()} (tol there {tol.ravel()[err.argmax()]})"


def posterior_params(k, d, seed):
    r = np.random.default_rng(seed)
    return {"alpha_log": (0.4 * r.normal(size=k)).astype(np.float32), "mus_loc": (2 * r.normal(size=(k, d))).astype(np.float32)}


# ------------------------------------------------------------------------------------------------ assignment
def assign_inputs(k, d, rows, seed=0):
    """The example's three clusters at -10, 10, -2 with scales 0.1, 1, 0.1, cycled (and shifted) over k components; rows drawn from
    them.  Returns float32 (obs (rows, d), mus (k, d), sigs (k, d), pis (k,))."""
    r = np.random.default_rng(1000 * k + 10 * d + rows + seed)
    j = np.arange(k)
    mus = (np.array([-10.0, 10.0, -2.0])[j % 3] + 0.37 * (j // 3))[:, None] + 0.01 * np.arange(d)[None, :]
    sigs = np.broadcast_to(np.array([0.1, 1.0, 0.1])[j % 3][:, None], (k, d))
    pis = r.uniform(0.5, 1.5, k)
    pis /= pis.sum()
    z = r.integers(0, k, rows)
    obs = mus[z] + sigs[z] * r.normal(size=(rows, d))
    return obs.astype(np.float32), mus.astype(np.float32), np.ascontiguousarray(sigs, np.float32), pis.astype(np.float32)


def a64(obs, mus, sigs, pis):
    """(a (rows, k) in float64 from the float32 inputs, its condition scale)."""
    x, m, s, p = (np.asarray(v, np.float64) for v in (obs, mus, sigs, pis))
    z = (x[:, None, :] - m[None]) / s[None]
    a = (-0.5 * z * z - np.log(s)[None] - HALF_LOG_2PI).sum(axis=2) + np.log(p)[None]
    scale = (0.5 * z * z + np.abs(np.log(s))[None] + HALF_LOG_2PI).sum(axis=2) + np.abs(np.log(p))[None]
    return a, scale


def a32_restated(obs, mus, sigs, pis):
    """The direct form in numpy float32, summed over c in index order."""
    x, m, s, p = (np.asarray(v, np.float32) for v in (obs, mus, sigs, pis))
    acc = np.zeros((x.shape[0], m.shape[0]), np.float32)
    for c in range(x.shape[1]):
        z = (x[:, None, c] - m[None, :, c]) / s[None, :, c]
        acc = acc + (np.float32(-0.5) * z * z - np.log(s[None, :, c]) - np.float32(HALF_LOG_2PI))
    return acc + np.log(p)[None]


def a_bound(scale):
    return A_BOUND_ULPS * 2.0 ** -24 * scale


def judged_rows(a, bound):
    """Rows whose float64 maximum leads every other component by more than the two bounds together (with one bound for all: a
    top-two gap above twice the bound); k = 1: every row."""
    best = a.argmax(axis=1)
    r = np.arange(a.shape[0])
    lead = a[r, best][:, None] - a - (bound[r, best][:, None] + bound)
    lead[r, best] = np.inf
    return (lead > 0).all(axis=1)


def logsumexp64(a):
    m = a.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(a - m).sum(axis=1, keepdims=True)))[:, 0]


# ------------------------------------------------------------------------------------------------ the outcome kernel's tile plan
def obs_tile_plan(rows, d, tp=T // 2, threads=256):
    """k_predict_gmm_obs's index arithmetic restated: per workgroup tp d pairs -- element e of the lower half
    and e + H of the upper, H = ceil(rows d / 2) -- walked by `threads` threads with the row and column carried incrementally.
    Returns (writes per element, writes per zs row, largest index into the two staged component arrays)."""
    n_tot = rows * d
    half = (n_tot + 1) // 2
    tile = tp * d
    wrote, zs = np.zeros(n_tot, int), np.zeros(rows, int)
    top = [0, 0]
    for b in range((half + tile - 1) // tile):
        P0 = b * tile
        npairs = min(tile, half - P0)
        eu0 = P0 + half
        rl0, ru0 = b * tp, eu0 // d
        staged = [set(), set()]
        for t in range(2 * tp + 1):
            hi, i = (1, t - tp) if t >= tp else (0, t)
            r = (ru0 if hi else rl0) + i
            if r < rows:
                staged[hi].add(i)
                e = r * d
                if (eu0 <= e < eu0 + npairs) if hi else (e < half):
                    zs[r] += 1
        cu0 = eu0 - ru0 * d
        for t in range(threads):
            rl, cl, ru, cu = t // d, t % d, (cu0 + t) // d, (cu0 + t) % d
            for p in range(t, npairs, threads):
                e0, e1 = P0 + p, P0 + p + half
                assert rl in staged[0] and (rl0 + rl) * d + cl == e0, (rows, d, b, t, p)
                wrote[e0] += 1
                top[0] = max(top[0], rl)
                if e1 < n_tot:
                    assert ru in staged[1] and (ru0 + ru) * d + cu == e1, (rows, d, b, t, p)
                    wrote[e1] += 1
                    top[1] = max(top[1], ru)
                cl, rl = cl + threads % d, rl + threads // d
                if cl >= d:
                    cl, rl = cl - d, rl + 1
                cu, ru = cu + threads % d, ru + threads // d
                if cu >= d:
                    cu, ru = cu - d, ru + 1
    return wrote, zs, top
