"""The float64 reference of d3p_column_moments and its DERIVED error bound: u = 2^-24, E = 2^-53, t = x - c exactly, T >=
|t|.  ASSUMED of the matrix instruction: every product and addition is rounded to nearest at most once, nothing underflows.  The shift
c may be a neighbour of float32(mean) (another order than numpy's): delta = 2 u mean|x| covers |c - mean|, T = |x - mean| + delta."""
import numpy as np

U, E = 2.0 ** -24, 2.0 ** -53


def geometry(lib, n, d):
    B, L, R = lib.d3p_column_moments_block_cols(), lib.d3p_column_moments_strip_rows(), lib.d3p_column_moments_segment_rows(n, d)
    return B, L, R, -(-n // R)


def reference(x):
    x64 = x.astype(np.float64)
    mean = x64.mean(axis=0)
    xc = x64 - mean
    return mean, xc.T @ xc


def bound(x, L, R, nseg):
    """(tolerance of mean (d,), tolerance of m2 (d, d)).  G: two roundings of t, one of the product and L additions in any order give
    K_u = L + 4; its float64 chain has A = R / L + ceil(nseg / 8) + 8 additions.  s is a float64 chain of A_s = R / 2 + 1 + ceil(nseg
    / 8) + 8 additions of fl32(t): u_s = u_t + (A_s + 1) E with u_t = u, or 0 for a column whose fl32(x - c) is EXACT for
    float32(mean) and both its neighbours (Sterbenz).  m2 = G - s_c s_e / n adds the cross terms of the s errors and float64
    roundings; the mean adds numpy's own pairwise rounding of the reference, (log2 n + 2) E mean|x|."""
    x64 = x.astype(np.float64)
    n = x64.shape[0]
    mean, mabs = x64.mean(axis=0), np.abs(x64).mean(axis=0)
    delta = 2.0 * U * mabs
    T = np.abs(x64 - mean) + delta
    TT, S1 = T.T @ T, T.sum(axis=0)
    chunks = -(-nseg // 8) + 8
    A, A_s, K_u = R // L + chunks, R // 2 + 1 + chunks, L + 4
    c32 = mean.astype(np.float32)
    exact = np.ones(x.shape[1], bool)
    for c in (c32, np.nextafter(c32, np.float32(np.inf)), np.nextafter(c32, np.float32(-np.inf))):
        exact &= ((x.astype(np.float32) - c).astype(np.float64) == x64 - c.astype(np.float64)).all(axis=0)
    u_s = np.where(exact, 0.0, U) + (A_s + 1) * E
    eta, s_abs = u_s * S1, n * delta
    cross = (np.outer(s_abs, eta) + np.outer(eta, s_abs) + np.outer(eta, eta)) / n
    tol_m2 = (K_u * U + (A + 2) * E) * TT + cross + 4.0 * E * (TT + np.outer(s_abs + eta, s_abs + eta) / n)
    return eta / n + 3.0 * E * (np.abs(mean) + delta) + (np.log2(n) + 2.0) * E * mabs, tol_m2


def exact_table(n, d, dtype, seed):
    """Columns 1000 (c + 1) + v, integer v in [-8, 8], rows in mirrored pairs v, -v (+ one of v = 0): (x, mean, m2), the moments exact."""
    v = np.random.default_rng(seed).integers(-8, 9, (n // 2, d))
    v = np.concatenate([np.stack([v, -v], axis=1).reshape(-1, d), np.zeros((n % 2, d), np.int64)])
    base = 1000 * (np.arange(d, dtype=np.int64) + 1)
    return (base + v).astype(dtype), base.astype(np.float64), (v.T @ v).astype(np.float64)
