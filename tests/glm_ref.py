"""Comparator for the regression families (logistic, linear, Poisson): the per-example ELBO written with ``torch.distributions``
in float64 on the CPU, differentiated by autograd -- the external truth DESIGN.md section 2 names for per-example gradients.

Only the per-example loss is stated here.  The guide noise comes from the oracle's streams (``O.px_eps``, the particle keys of
tests/particles_ref.py), and the step after the per-example rows is the oracle's own family-agnostic stages
(``O.clip_rows`` -> ``O.combine`` -> ``O.perturb`` -> ``O.adam``): the step rule is the reference's, not restated.

For family = "logistic" ``px_loss_grads`` must reproduce ``O.logreg_px_grads`` (pinned since round 1): tests/test_glm_host.py
checks that on the CPU, so every GPU comparison below rests on a helper that was itself checked against something independent.

Tolerances: per-example rows and losses 2e-5 of the row scale, batch gradients 1e-4 (+ 1e-6 max), parameters
after Adam 1e-5, 20-step trajectories 5e-5 (losses) / 2e-4 (parameters), keys bit-exact.

Poisson: exp(t) multiplies the dot product's rounding error by e^t, and dl = exp(t) - y cancels where the rate is close to the count
(t = 0.0013, y = 1: exp(t) - y = 0.0013, one ulp of exp(t) is 5e-5 of it).  The Poisson bound on per-example GRADIENTS is therefore wider than
2e-5, and it is not taken from the device: it is four times the float32 error of the comparator itself.  ``float32_calibration``
evaluates the same ELBO through float32 torch against the float64 one over the inputs of the per-example sweep (``sweep_cases``:
the seeds, masks, guides and noise sources tests/test_gpu_glm.py::test_px_grads_at_every_width runs), in the form of the project's
check (|a - b| <= rtol |b| + 0.1 rtol max|b|).  Smallest passing rtol, on the CPU (tests/test_glm_host.py recomputes the Poisson
figure and asserts it stays at or below the 3.5e-5 the bound is built on):

    Poisson  gradients 3.496e-05 (worst at d = 1024 + intercept, B = 1: the cancelling row above)   losses 7.142e-07
    linear   gradients 4.572e-06                                                                    losses 3.754e-07

POISSON_GRAD_TOL = 4 x 3.496e-05 = 1.4e-4 (the factor 4 is the margin tests/predictive_ref.py gives its product bound).  Poisson
losses (lgammaf included) and everything of the linear family stay at the project's 2e-5."""
import math
from types import SimpleNamespace

import numpy as np
import torch

FAMILIES = ("logistic", "linear", "poisson")
PX_TOL = 2e-5
POISSON_GRAD_TOL = 4 * 3.496e-05


def hyper(d, intercept=False, prior_w=1.0, prior_b=1.0, lik_scale=1.0, obs_scale=1.0, sigma=1.0):
    """What the per-example loss needs from the model and the state: lik_scale = plate scale N, obs_scale = observation_scale."""
    return SimpleNamespace(d=int(d), intercept=bool(intercept), prior_w=float(prior_w), prior_b=float(prior_b),
                           lik_scale=float(lik_scale), obs_scale=float(obs_scale), sigma=float(sigma))


def _scale(unc, guide):
    return torch.exp(unc) if guide == "exp" else torch.nn.functional.softplus(unc)


def _loglik(family, t, y, sigma):
    import torch.distributions as D
    if family == "logistic":
        return D.Bernoulli(logits=t).log_prob(y)
    if family == "linear":
        return D.Normal(t, torch.as_tensor(sigma, dtype=t.dtype)).log_prob(y)
    if family == "poisson":
        return D.Poisson(torch.exp(t), validate_args=False).log_prob(y)
    raise ValueError(family)


def _elbo_rows(family, h, loc, unc, X, y, eps, guide):
    """-(N log p(y_i | x_i, z_i) + log p(z_i) - log q(z_i)) / obs_scale per row; loc / unc are (B, D) leaves (one copy per example)."""
    import torch.distributions as D
    dt = loc.dtype
    s = _scale(unc, guide)
    z = loc + s * eps
    prior = torch.cat([torch.full((h.d,), h.prior_w, dtype=dt), torch.full((int(h.intercept),), h.prior_b, dtype=dt)])
    logq = D.Normal(loc, s).log_prob(z).sum(-1)
    logp = D.Normal(torch.zeros((), dtype=dt), prior).log_prob(z).sum(-1)
    t = (X * z[:, :h.d]).sum(-1)
    if h.intercept:
        t = t + z[:, h.d]
    ll = _loglik(family, t, y, h.sigma)
    return ((logq - logp) - h.lik_scale * ll) / h.obs_scale, t


def px_loss_grads(family, h, loc, unc, Xb, yb, eps, mask=None, guide="softplus", dtype=torch.float64, return_t=False):
    """Per-example losses (B) and gradients (B, 2 D) = [d/dloc | d/dunc], as svi.py:271-306 scales them: rows of masked-out examples
    are zero, losses are multiplied by obs_scale * factor, factor = B / n (0 if n == 0).  eps: (B, D), or (B, K, D) for K particles
    (mean of the particles' losses and gradients).  Returns (losses, grads, n, factor) as float64 numpy arrays."""
    B, D = Xb.shape[0], h.d + int(h.intercept)
    eps = np.asarray(eps)
    if eps.ndim == 2:
        eps = eps[:, None, :]
    K = eps.shape[1]
    X, y = torch.tensor(np.asarray(Xb), dtype=dtype), torch.tensor(np.asarray(yb), dtype=dtype)
    L = torch.zeros(B, dtype=dtype)
    G = torch.zeros(B, 2 * D, dtype=dtype)
    tmax = 0.0
    for q in range(K):
        lb = torch.tensor(np.asarray(loc), dtype=dtype).expand(B, D).clone().requires_grad_(True)
        ub = torch.tensor(np.asarray(unc), dtype=dtype).expand(B, D).clone().requires_grad_(True)
        rows, t = _elbo_rows(family, h, lb, ub, X, y, torch.tensor(eps[:, q], dtype=dtype), guide)
        rows.sum().backward()
        L += rows.detach()
        G += torch.cat([lb.grad, ub.grad], dim=1)
        tmax = max(tmax, float(t.detach().abs().max()))
    L, G = (L / K).numpy().astype(np.float64), (G / K).numpy().astype(np.float64)
    m = np.ones(B) if mask is None else np.asarray(mask, np.float64)
    n = int((m != 0).sum())
    factor = 0.0 if n == 0 else B / n
    out = (L * m * h.obs_scale * factor, G * m[:, None], n, factor)
    return out + (tmax,) if return_t else out


def row_errors(got, ref):
    """max_j |got_ij - ref_ij| / max_j |ref_ij| per row (rows of zeros: the absolute error)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.ndim == 1:
        got, ref = got[:, None], ref[:, None]
    scale = np.abs(ref).max(axis=1)
    return np.abs(got - ref).max(axis=1) / np.where(scale > 0, scale, 1.0)


def smallest_passing_rtol(got, ref):
    """The smallest rtol at which the project's per-example check |a - b| <= rtol |b| + 0.1 rtol max|b| passes."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (np.abs(ref) + 0.1 * np.abs(ref).max())).max()) if np.abs(ref).max() > 0 else 0.0


# ---------------------------------------------------------------- the per-example sweep's inputs (tests/test_gpu_glm.py and the calibration)
SWEEP_WIDTHS = (1, 4, 64, 128, 129, 192, 256, 257, 511, 512, 1023, 1024, 2048, 2056)
SWEEP_SIGMA = {"logistic": 1.0, "linear": 0.5, "poisson": 1.0}
SWEEP_N = 10 ** 4


def sweep_hyper(family, d, intercept):
    return hyper(d, intercept, prior_w=1.5, prior_b=2.5, lik_scale=SWEEP_N, obs_scale=SWEEP_N, sigma=SWEEP_SIGMA[family])


def sweep_cases(O, family, d, intercept):
    """(B, guide, onchip, seed, X, y, loc, unc, mask, eps) for B in {1, 33, 200, 4096 (d <= 512)}: the guide transform and the noise
    source (memory / the oracle's key stream) alternate over the batch sizes and start from another combination at every (d, intercept)."""
    combos = [("softplus", True), ("exp", False), ("softplus", False), ("exp", True)]
    D = d + int(intercept)
    for i, B in enumerate([1, 33, 200] + ([4096] if d <= 512 else [])):
        guide, onchip = combos[(i + SWEEP_WIDTHS.index(d) + int(intercept)) % 4]
        seed = 1000 * d + 10 * B + int(intercept)
        X, y, loc, unc = problem(family, B, d, intercept, seed, SWEEP_SIGMA[family])
        mask = np.random.default_rng(seed + 1).random(B) < 0.8
        if B == 1:
            mask[:] = True
        eps = (O.px_eps(O.convert_to_jax_rng_key(O.PRNGKey(seed)), B, D) if onchip
               else np.random.default_rng(seed + 2).normal(size=(B, D)).astype(np.float32))
        yield B, guide, onchip, seed, X, y, loc, unc, mask, eps


def float32_calibration(O, family, widths=SWEEP_WIDTHS):
    """The reference's OWN float32 error on the sweep's inputs: the same ELBO through float32 torch autograd against the float64 one,
    as the smallest passing rtol of the project's check.  Returns (gradients, losses, (d, intercept, B) of the worst gradient case)."""
    wg = wl = 0.0
    where = None
    for d in widths:
        for intercept in (False, True):
            h = sweep_hyper(family, d, intercept)
            for B, guide, onchip, seed, X, y, loc, unc, mask, eps in sweep_cases(O, family, d, intercept):
                L64, G64, _, _ = px_loss_grads(family, h, loc, unc, X, y, eps, mask, guide)
                L32, G32, _, _ = px_loss_grads(family, h, loc, unc, X, y, eps, mask, guide, dtype=torch.float32)
                g = smallest_passing_rtol(G32, G64)
                if g > wg:
                    wg, where = g, (d, intercept, B)
                wl = max(wl, smallest_passing_rtol(L32, L64))
    return wg, wl, where


# ---------------------------------------------------------------- noise streams (the oracle's; particle keys as tests/particles_ref.py)
def px_eps(O, jax_key, B, D, K=1):
    if K == 1:
        return O.px_eps(jax_key, B, D)
    from tests import particles_ref as R
    return R.px_eps(O, jax_key, B, D, K)


class State:
    """Mutable mirror of DPSVIState (key, [loc | unc], Adam moments, step counter)."""

    def __init__(self, key, loc, unc):
        self.key = np.asarray(key, np.uint32).reshape(16).copy()
        self.params = np.concatenate([loc, unc]).astype(np.float32)
        self.m = np.zeros_like(self.params)
        self.v = np.zeros_like(self.params)
        self.step = 0


def step(O, family, h, hy, st, Xb, yb, mask=None, guide="softplus", K=1, eps=None):
    """One DPSVI.update with the key schedule of O.logreg_update: (next, gradient, perturbation) = split(key, 3); per-example rows
    from ``px_loss_grads``; then the oracle's clip, mean, perturbation (one key per parameter leaf) and Adam.  Advances ``st``;
    returns (loss, perturbed gradient)."""
    D = h.d + int(h.intercept)
    B = Xb.shape[0]
    ks = O.split(st.key, 3)
    jax_key = O.convert_to_jax_rng_key(ks[1])
    if eps is None:
        eps = px_eps(O, jax_key, B, D, K)
    L, G, n, f = px_loss_grads(family, h, st.params[:D], st.params[D:], Xb, yb, eps, mask, guide)
    clipped = O.clip_rows(G.astype(np.float32), hy.clip)
    loss, avg = O.combine(clipped, L.astype(np.float32))
    g = O.perturb(ks[2], avg, [D, D], hy.dp_scale, hy.clip, float(n), h.obs_scale, f)
    st.params, st.m, st.v = O.adam(st.params, st.m, st.v, g, st.step, lr=hy.lr, b1=hy.b1, b2=hy.b2, eps=hy.adam_eps)
    st.step += 1
    st.key = np.asarray(ks[0], np.uint32).reshape(16).copy()
    return loss, g


def evaluate(O, family, h, loc, unc, Xb, yb, jax_key, guide="softplus"):
    """DPSVI.evaluate at the evaluate key rule: eps = normal(split(split(split(jax_key)[1])[1])[1]), ONE guide
    draw for the whole batch, plate(N, B) scales the likelihood by N / B; -ELBO in float64."""
    import torch.distributions as Dist
    D = h.d + int(h.intercept)
    B = Xb.shape[0]
    k = O.tf_split(O.tf_split(jax_key)[1])[1]
    eps = torch.tensor(O.tf_normal(O.tf_split(k)[1], D), dtype=torch.float64)
    loc, unc = torch.tensor(np.asarray(loc), dtype=torch.float64), torch.tensor(np.asarray(unc), dtype=torch.float64)
    s = _scale(unc, guide)
    z = (loc.float() + s.float() * eps.float()).double()      # (z is formed in float32 by every implementation, the oracle included)
    prior = torch.cat([torch.full((h.d,), h.prior_w, dtype=torch.float64), torch.full((int(h.intercept),), h.prior_b, dtype=torch.float64)])
    logq = (-0.5 * eps * eps - torch.log(s) - 0.5 * math.log(2 * math.pi)).sum()
    logp = Dist.Normal(torch.zeros((), dtype=torch.float64), prior).log_prob(z).sum()
    t = torch.tensor(np.asarray(Xb), dtype=torch.float64) @ z[:h.d] + (z[h.d] if h.intercept else 0.0)
    ll = _loglik(family, t, torch.tensor(np.asarray(yb), dtype=torch.float64), h.sigma).sum()
    return float(-(logp + (h.lik_scale / B) * ll - logq))


# ---------------------------------------------------------------- test problems: X ~ N(0, 1) / sqrt(d), |w| such that |t| <= 4
def problem(family, B, d, intercept, seed, sigma=1.0):
    """(X, y, loc, unc): features N(0, 1) / sqrt(d), loc of norm ~1.5 (so t = x . z stays well inside |t| <= 4), unc ~ -1.5."""
    r = np.random.default_rng(seed)
    D = d + int(intercept)
    X = (r.normal(size=(B, d)) / math.sqrt(d)).astype(np.float32)
    w = r.normal(size=D)
    loc = (1.5 * w / np.linalg.norm(w)).astype(np.float32)
    unc = (-1.5 + 0.3 * r.normal(size=D)).astype(np.float32)
    t = X.astype(np.float64) @ loc[:d] + (loc[d] if intercept else 0.0)
    if np.abs(t).max() > 2.0:       # (narrow rows: one feature of 4 sigma; keeps |t| <= 4 with the guide noise s eps x on top)
        loc = (loc * (2.0 / np.abs(t).max())).astype(np.float32)
        t = X.astype(np.float64) @ loc[:d] + (loc[d] if intercept else 0.0)
    if family == "logistic":
        y = (r.random(B) < 1.0 / (1.0 + np.exp(-t))).astype(np.float32)
    elif family == "linear":
        y = (t + sigma * r.normal(size=B)).astype(np.float32)
    else:
        y = r.poisson(np.exp(t)).astype(np.float32)
    return X, y, loc, unc
