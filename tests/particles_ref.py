"""Comparator for multi-particle ELBO gradients (Trace_ELBO(num_particles=K)), composed from the oracle's existing entry points.

The particle rule is restated here with the oracle's threefry functions; everything else -- per-example
gradients, clip, mean, perturbation, Adam, the batch-level evaluate -- is the oracle's own.  At K = 1 each function reduces to
the oracle's single-particle path (tests/test_gpu_particles.py anchors that bit for bit)."""
import numpy as np


def particle_key(O, jax_key, B, p, K, q):
    """split(split(jax_key, B)[p], K)[q]; K == 1: split(jax_key, B)[p]."""
    k = O.tf_split(jax_key, B)[p]
    return k if K == 1 else O.tf_split(k, K)[q]


def sample_key(O, pkey):
    """The one-site guide's sample key: split(split(particle key)[1])[1]."""
    return O.tf_split(O.tf_split(pkey)[1])[1]


def px_eps(O, jax_key, B, D, K):
    """(B, K, D) guide noise of a one-site guide."""
    return np.stack([np.stack([O.tf_normal(sample_key(O, particle_key(O, jax_key, B, p, K, q)), D) for q in range(K)])
                     for p in range(B)]).astype(np.float32)


def px_eps_sites(O, jax_key, B, sizes, K):
    """(B, K, sum(sizes)): per particle, numpyro's seed handler over the sample sites (rng, site_key = split(rng))."""
    out = np.empty((B, K, int(sum(sizes))), np.float32)
    for p in range(B):
        for q in range(K):
            rng = O.tf_split(particle_key(O, jax_key, B, p, K, q))[1]
            off = 0
            for n in sizes:
                rng, site = O.tf_split(rng)
                out[p, q, off:off + n] = O.tf_normal(site, n)
                off += n
    return out


def px_grads(O, spec, loc, unc, Xb, yb, eps, mask=None):
    """Per-example loss and gradient averaged over the particles of eps (B, K, D), in float64 before the float32 result."""
    K = eps.shape[1]
    m = None if mask is None else np.asarray(mask, np.float32)
    Ls, Gs = [], []
    n = f = None
    for q in range(K):
        L, G, n, f = O.logreg_px_grads(spec, loc, unc, Xb, yb, np.ascontiguousarray(eps[:, q]), m)
        Ls.append(L.astype(np.float64))
        Gs.append(G.astype(np.float64))
    return (np.mean(Ls, axis=0).astype(np.float32), np.mean(Gs, axis=0).astype(np.float32), n, f)


def update(O, spec, hyper, st, Xb, yb, K, mask=None, eps_fn=None):
    """One DPSVI.update with K particles, the key schedule of O.logreg_update: (next, gradient, perturbation) = split(key, 3),
    jax key = convert(gradient key), then clip, mean, perturbation (one key per parameter leaf) and Adam.  Advances `st`;
    returns (loss, perturbed gradient)."""
    D = spec.d + spec.intercept
    ks = O.split(st.key, 3)
    jax_key = O.convert_to_jax_rng_key(ks[1])
    B = Xb.shape[0]
    eps = px_eps(O, jax_key, B, D, K) if eps_fn is None else eps_fn(jax_key, B)
    L, G, n, f = px_grads(O, spec, st.params[:D], st.params[D:], Xb, yb, eps, mask)
    clipped = O.clip_rows(G, hyper.clip)
    loss, avg = O.combine(clipped, L)
    g = O.perturb(ks[2], avg, [D, D], hyper.dp_scale, hyper.clip, float(n), 1.0 / spec.inv_obs, f)
    st.params, st.m, st.v = O.adam(st.params, st.m, st.v, g, st.step.value, lr=hyper.lr, b1=hyper.b1, b2=hyper.b2,
                                   eps=hyper.adam_eps)
    st.step.value += 1
    st.key = np.asarray(ks[0], np.uint32).reshape(16).copy()
    return loss, g


def evaluate(O, spec, loc, unc, Xb, yb, jax_key, K):
    """DPSVI.evaluate with K particles: the mean over q of O.logreg_evaluate at split(jax_key, K)[q] (K == 1: jax_key)."""
    if K == 1:
        return O.logreg_evaluate(spec, loc, unc, Xb, yb, jax_key)
    keys = O.tf_split(jax_key, K)
    return float(np.mean([O.logreg_evaluate(spec, loc, unc, Xb, yb, keys[q]) for q in range(K)]))


def meanfield_evaluate(O, spec, params_tree, Xb, yb, jax_key, K):
    if K == 1:
        return O.meanfield_logreg_evaluate(spec, params_tree, Xb, yb, jax_key)
    keys = O.tf_split(jax_key, K)
    return float(np.mean([O.meanfield_logreg_evaluate(spec, params_tree, Xb, yb, keys[q]) for q in range(K)]))


def meanfield_update(O, spec, hyper, st, Xb, yb, K, mask=None):
    """O.meanfield_logreg_update with K particles: per particle the two sites' eps ('w' then 'intercept'), the mean
    per-example gradient in tree order, joint clip, mean, one perturbation key per leaf, Adam.  Advances `st` (an
    O.MeanFieldLogregState); returns (loss, perturbed gradient in tree order)."""
    d = spec.d
    D = d + 1
    ks = O.split(st.key, 3)
    jax_key = O.convert_to_jax_rng_key(ks[1])
    B = Xb.shape[0]
    eps = px_eps_sites(O, jax_key, B, [d, 1], K)
    perm = O.MeanFieldLogregState.tree_from_kernel(d)
    kern = np.empty(2 * D, np.float32)
    kern[perm] = st.params
    L, G, n, f = px_grads(O, spec, kern[:D], kern[D:], Xb, yb, eps, mask)
    clipped = O.clip_rows(np.ascontiguousarray(G[:, perm]), hyper.clip)
    loss, avg = O.combine(clipped, L)
    g = O.perturb(ks[2], avg, O.MeanFieldLogregState.leaf_sizes(d), hyper.dp_scale, hyper.clip, float(n), 1.0 / spec.inv_obs, f)
    st.params, st.m, st.v = O.adam(st.params, st.m, st.v, g, st.step, lr=hyper.lr, b1=hyper.b1, b2=hyper.b2, eps=hyper.adam_eps)
    st.step += 1
    st.key = np.asarray(ks[0], np.uint32).reshape(16).copy()
    return loss, g
