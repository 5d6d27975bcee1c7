"""Comparator of the label sums and the energy distance's permutation test (d3p_amd/permutation.py, d3p_amd/csrc/d3p_label_sums.hip;
DESIGN.md section 4y): a numpy restatement of the kernel's rule IN ITS STATED ORDER on the float32 distances of tests/fidelity_ref.py's
emulation, an exact comparator (float64 distances, math.fsum), the derived bound, and the test's closing arithmetic.  Nothing here
reaches a device.

    pack(bits)                      (R, m) bool -> (ceil(m / 32), R) uint32 label words, tile-major
    unpack(labels, m)               the inverse, the bits of rows >= m ignored
    distances32(z)                  (m, m) float64 holding the kernel's float32 distances
    restate(z, labels, row_sum)     -> {"s11", "s1t", "n1"} in exactly the kernel's order of float64 additions
    exact(z, labels)                -> (R,) float64: fsum over the selected pairs of the float64 distances
    chain(m), bound(ex, m, d)       A of the order, and the largest |s11 - exact| the rule admits
    statistics(s11, s1t, n1, total, m) -> (d2, statistic);  p_value(stat) -> (n_ge, p)
    energy_test(x, y, labels)       the whole test on the restatement

THE ORDER (the header of d3p_label_sums.hip): rows in tiles of T = 32, tile J in slot J mod 4.  Per (tile pair (I, J), labelling) and
row ii of tile I the row sum adds the 32 distances in ascending column onto 0, a clear column bit adding +0.0; per (I, slot) the slot
sum adds the row sums of set row bits (a clear one adds +0.0) in ascending ii, then ascending J, onto 0; the four slot sums are added in
ascending order onto 0 (the cell); the cells are added in ascending I onto 0.

THE BOUND.  Every summand is non-negative, so every error is relative.  A distance carries rho = (d / 2 + 2) 2^-24 (1 + 2^-10) (DESIGN.md
4v; its widening to float64 is exact).  A float64 sum of non-negative terms errs by at most (the number of additions on the longest
chain a term passes through) x 2^-53, to first order.  A distance passes through at most: the 32 additions of its row sum; one
addition per (tile of its slot, row) of the slot sum, 32 ceil(tiles / 4); the 4 additions of the slots; the `tiles` additions of the
cells.  So A = 32 + 32 ceil(tiles / 4) + 4 + tiles, and with 2 more for the second-order terms (A 2^-53 < 2^-30 for every admissible
m):

    |s11 - exact| <= (rho + (A + 2) 2^-53) exact
"""
import numpy as np

from tests import fidelity_ref as FR
from tests.energy_ref import U64, _fsum, _q32

T = 32
SLOTS = 4
S = T * SLOTS          # the rows after which a slot takes its second tile: the order's next level


def _as2(t):
    t = np.asarray(t)
    return t[:, None] if t.ndim == 1 else t


def pack(bits):
    bits = np.asarray(bits, bool)
    R, m = bits.shape
    tiles = -(-m // T)
    full = np.zeros((R, tiles * T), np.uint64)
    full[:, :m] = bits
    words = (full.reshape(R, tiles, T) << np.arange(T, dtype=np.uint64)).sum(axis=2)
    return np.ascontiguousarray(words.T.astype(np.uint32))


def unpack(labels, m):
    labels = np.asarray(labels, np.uint32)
    tiles, R = labels.shape
    assert tiles == -(-m // T)
    bits = (labels.T[:, :, None] >> np.arange(T, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(R, tiles * T)[:, :m].astype(bool)


def distances32(z):
    z = _as2(z)
    with np.errstate(all="ignore"):
        return np.sqrt(_q32(z[:, None, :], z[None, :, :])).astype(np.float32).astype(np.float64)


def _finite(z):
    return bool(np.isfinite(_as2(z).astype(np.float64)).all())


def restate(z, labels, row_sum):
    """The kernel's outputs in the kernel's order, vectorised over the labellings (which never meet)."""
    z = _as2(z)
    m = z.shape[0]
    g = unpack(labels, m)                       # (R, m)
    R = g.shape[0]
    tiles = -(-m // T)
    D = np.zeros((tiles * T, tiles * T), np.float64)
    D[:m, :m] = distances32(z)
    G = np.zeros((R, tiles * T), bool)
    G[:, :m] = g
    s11 = np.zeros(R, np.float64)
    with np.errstate(all="ignore"):
        for I in range(tiles):
            slots = []
            for w in range(SLOTS):
                acc = np.zeros(R, np.float64)
                for J in range(w, tiles, SLOTS):
                    tile = D[I * T:(I + 1) * T, J * T:(J + 1) * T]
                    row = np.zeros((T, R), np.float64)         # the 32 row sums at once: each is its own chain over jj
                    for jj in range(T):
                        row = row + np.where(G[None, :, J * T + jj], tile[:, jj][:, None], 0.0)
                    for ii in range(T):
                        acc = acc + np.where(G[:, I * T + ii], row[ii], 0.0)
                slots.append(acc)
            cell = np.zeros(R, np.float64)
            for acc in slots:
                cell = cell + acc
            s11 = s11 + cell
    if not _finite(z):
        s11 = np.full(R, np.nan)
    row_sum = np.asarray(row_sum, np.float64)
    s1t = np.zeros(R, np.float64)
    with np.errstate(all="ignore"):
        for i in range(m):
            s1t = np.where(g[:, i], s1t + row_sum[i], s1t)
    return {"s11": s11, "s1t": s1t, "n1": g.sum(axis=1).astype(np.int64)}


def exact(z, labels):
    z = _as2(z).astype(np.float64)
    m = z.shape[0]
    g = unpack(labels, m)
    if not _finite(z):
        return np.full(g.shape[0], np.nan)
    D = np.sqrt(FR._q64(z, z))
    return np.array([_fsum(D[np.ix_(row, row)]) for row in g])


def chain(m):
    tiles = -(-m // T)
    return T + T * (-(-tiles // SLOTS)) + SLOTS + tiles


def bound(ex, m, d):
    return (FR.rho(d) + (chain(m) + 2.0) * U64) * np.abs(np.asarray(ex, np.float64))


def row_sums(z):
    """t_i of the pooled table by fidelity_ref's emulation (fsum: the device's order differs, within fidelity_ref.bound)."""
    z = _as2(z)
    return FR.emulate(z, z, True)["sum"]


def statistics(s11, s1t, n1, total, m):
    s11, s1t, n1 = np.asarray(s11, np.float64), np.asarray(s1t, np.float64), np.asarray(n1, np.float64)
    n0 = float(m) - n1
    with np.errstate(all="ignore"):
        s10 = s1t - s11
        s00 = total - 2.0 * s10 - s11
        d2 = 2.0 * s10 / (n1 * n0) - s11 / (n1 * n1) - s00 / (n0 * n0)
        return d2, n1 * n0 / (n1 + n0) * d2


def p_value(stat):
    stat = np.asarray(stat, np.float64)
    n_ge = int((stat[1:] >= stat[0]).sum())
    return n_ge, (1 + n_ge) / stat.shape[0]


def brute(D, g):
    """(d2, statistic) of one labelling by the sums over the three blocks of the distance matrix D."""
    g = np.asarray(g, bool)
    n1, n0 = int(g.sum()), int((~g).sum())
    s11, s00, s10 = _fsum(D[np.ix_(g, g)]), _fsum(D[np.ix_(~g, ~g)]), _fsum(D[np.ix_(g, ~g)])
    d2 = 2.0 * s10 / (n1 * n0) - s11 / (n1 * n1) - s00 / (n0 * n0)
    return d2, n1 * n0 / (n1 + n0) * d2


def energy_test(x, y, labels):
    """The test on the pooled table [x; y] under `labels` (column 0 the identity), by the restatement: {"d2", "statistic" (all
    labellings), "n_ge", "p_value", "s11", "s1t", "n1"}."""
    z = np.concatenate([_as2(x), _as2(y)], axis=0)
    t = row_sums(z)
    out = restate(z, labels, t)
    d2, stat = statistics(out["s11"], out["s1t"], out["n1"], _fsum(t), z.shape[0])
    n_ge, p = p_value(stat)
    out.update(d2=d2, statistic=stat, n_ge=n_ge, p_value=p)
    return out
