"""numpy float64 restatement of d3p_stacking_weights and d3p_bb_pseudo_bma (include/d3p_hip.h): the same EM iteration
with the same start and stopping rule, and the bootstrap's weight stream rebuilt from threefry2x32 and the float32 uniform rule.  A
plain module (no test in it): tests/test_model_weights_host.py and tests/test_gpu_model_weights.py import it.

``threefry2x32`` here is a vectorised restatement of Random123's threefry2x32-20; the host test pins it word for word against
``oracle.threefry2x32``.
"""
import numpy as np

_ROT = ((13, 15, 26, 6), (17, 29, 16, 24))


def threefry2x32(k0, k1, c0, c1):
    """(o0, o1) of threefry2x32-20 for uint32 arrays of counters (broadcast against each other)."""
    k0, k1 = np.uint32(k0), np.uint32(k1)
    ks = (k0, k1, np.uint32(k0 ^ k1 ^ np.uint32(0x1BD11BDA)))
    c0, c1 = np.broadcast_arrays(np.asarray(c0, np.uint32), np.asarray(c1, np.uint32))
    with np.errstate(over="ignore"):
        x0, x1 = c0 + ks[0], c1 + ks[1]
        for i in range(5):
            for r in _ROT[i % 2]:
                x0 = x0 + x1
                x1 = (x1 << np.uint32(r)) | (x1 >> np.uint32(32 - r))
                x1 = x1 ^ x0
            x0 = x0 + ks[(i + 1) % 3]
            x1 = x1 + ks[(i + 2) % 3] + np.uint32(i + 1)
    return x0, x1


def bits_to_uniform(bits):
    """jax.random.uniform's float32 construction on [0, 1): (bits >> 9) | 0x3f800000 as a float, minus 1."""
    f = ((np.asarray(bits, np.uint32) >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    return np.maximum(np.float32(0.0), f)


def bb_bits(key, B, rows, b0=0):
    """The (B, rows) uint32 words of replicates b0 .. b0 + B - 1: word (r & 1) of threefry2x32(key, (r >> 1, b))."""
    r = np.arange(rows, dtype=np.uint64)
    b = np.arange(b0, b0 + B, dtype=np.uint32)[:, None]
    o0, o1 = threefry2x32(key[0], key[1], (r >> np.uint64(1)).astype(np.uint32)[None, :], b)
    return np.where((r & np.uint64(1)).astype(bool)[None, :], o1, o0)


def bb_weights(key, B, rows, b0=0):
    """g[b, r] = -log(1 - u) in float64 from the exact float32 u (1 - u is exact in float32)."""
    u = bits_to_uniform(bb_bits(key, B, rows, b0))
    return -np.log((np.float32(1.0) - u).astype(np.float64))


def _bad_rows(e):
    return bool((np.isnan(e) | (e == np.inf)).any() or (e == -np.inf).all(axis=0).any())


def stacking(e, tol=1e-7, max_iter=20000, history=False):
    """(w, n_iter, converged, gap, f[, gaps]) by the header's rule; e is (M, rows), float32 values."""
    e = np.asarray(e, np.float32).astype(np.float64)
    M, rows = e.shape
    w = np.full(M, 1.0 / M)
    gaps = []
    with np.errstate(all="ignore"):
        mx = e.max(axis=0)
        p = np.exp(e - mx)
        j = 0
        while True:
            den = np.zeros(rows)
            for k in range(M):
                den = den + w[k] * p[k]
            g = (p / den).sum(axis=1) / rows
            f = (mx + np.log(den)).sum()
            nan = bool(np.isnan(g).any())
            gap = np.nan if nan else g.max() - 1.0
            gaps.append(gap)
            converged = bool(gap <= tol)
            if converged or nan or j >= max_iter:
                if nan:
                    w, f = np.full(M, np.nan), np.nan
                out = (w, j, converged, gap, f)
                return out + (gaps,) if history else out
            w = w * g
            j += 1


def stacking_gap(e, w):
    """The duality gap max_m g_m - 1 of ANY w, in float64 from e: the certificate."""
    e = np.asarray(e, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        p = np.exp(e - e.max(axis=0))
        den = (np.asarray(w, np.float64)[:, None] * p).sum(axis=0)
        return (p / den).sum(axis=1).max() / e.shape[1] - 1.0


def bb_pseudo_bma(key, e, B, b0=0):
    """(w, z, scale): z is (B, M); scale[b] = rows sum_r g |e| / S_b over the finite e, the magnitude the test's bound is stated in."""
    e = np.asarray(e, np.float32).astype(np.float64)
    M, rows = e.shape
    g = bb_weights(key, B, rows, b0)
    with np.errstate(all="ignore"):
        S = g.sum(axis=1)
        T = np.empty((B, M))
        A = np.zeros(B)
        for m in range(M):
            term = np.where(g == 0.0, 0.0, g * e[m][None, :])
            T[:, m] = term.sum(axis=1)
            A = np.maximum(A, np.where(np.isfinite(term), np.abs(term), 0.0).sum(axis=1))
        z = rows * T / S[:, None]
        if _bad_rows(e):
            z = np.full((B, M), np.nan)
        ex = np.exp(z - z.max(axis=1, keepdims=True))
        wb = ex / ex.sum(axis=1, keepdims=True)
        w = wb.sum(axis=0) / B
    return w, z, rows * A / S
