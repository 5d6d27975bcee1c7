"""A permutation test for the two-sample energy distance of a synthetic table against a real one: where the
observed ``d2`` of ``d3p_amd.fidelity.energy_distance`` falls among the values that random relabellings of the pooled rows give.

    permutation_labels(n_x, n_y, n_perm, seed=0, device=None) -> (ceil(m / 32), n_perm + 1) uint32, m = n_x + n_y
    label_sums(z, labels, row_sum=None)                       -> LabelSums(s11, s1t, n1, total, m)
    energy_test(x, y, n_perm=999, seed=0)                     -> EnergyTest(d2, statistic, p_value, n_perm, null_mean, null_quantiles,
                                                                            n_ge, n_x, n_y, dim)

PRIVACY.  Every number here is computed from the PRIVATE table, without noise.  Releasing a p-value, or choosing a model by looking at
it, is NOT covered by the accountant (``DPSVI.get_epsilon``): the accountant covers the noised steps of training and nothing else.  The
functions are a diagnostic for the person who holds the data.

A bare ``d2`` cannot be read: "0.0031 to train, 0.0034 to test" does not say whether the synthetic table differs from the real one by
more than two fresh samples of one distribution would.  The test of Szekely & Rizzo (R's ``energy::eqdist.etest``) pools the tables,
``z = [x; y]`` with ``m = n_x + n_y`` rows, relabels the rows at random ``n_perm`` times and recomputes the statistic each time.  With
``D_ij`` the float32 distance of ``d3p_amd.fidelity``, ``t_i = sum_j D_ij`` (``fidelity.pair_stats(z, z, True)["sum"]``), ``T = sum_i
t_i`` and a labelling ``g`` in ``{0, 1}^m`` (1: "counts as y") with ``n1 = sum_i g_i`` and ``n0 = m - n1``:

    s11 = sum_{i,j} g_i g_j D_ij          s1t = sum_i g_i t_i
    S10 = s1t - s11                       S00 = T - 2 S10 - s11
    d2  = 2 S10 / (n1 n0) - s11 / n1^2 - S00 / n0^2            statistic = n1 n0 / (n1 + n0) d2

Per labelling only the quadratic form ``s11`` needs the pairs.  ``d3p_pair_label_sums`` (``d3p_amd/csrc/d3p_label_sums.hip``) computes
it for every labelling in ONE walk over the pairs: each distance is computed once and fed to every labelling while it lies in LDS --
never the ``m x m`` matrix, never a walk per labelling.  ``s11[r]`` is deterministic to the bit and depends on ``z`` and labelling ``r``
alone (the kernel's header states its order of summation).

Labelling 0 is the identity (rows ``>= n_x`` carry the 1), so the observed statistic comes from the same kernel, the same distances and
the same order as the null ones: like is compared with like.  THE P-VALUE CONVENTION is the one that counts the observed labelling among
the relabellings, so it is never 0:

    n_ge = #{r >= 1 : statistic_r >= statistic_0}            p_value = (1 + n_ge) / (n_perm + 1)

and a TIE COUNTS as ``>=``.  ``d2`` and ``statistic`` are float64 torch arithmetic on the kernel's sums and carry no bit promise;
``n_ge`` and ``p_value`` are the count.  ``null_mean`` and ``null_quantiles`` (0.5, 0.95, 0.99; ``torch.quantile``) describe
``statistic_r`` over ``r >= 1``.

WHAT THE TEST DOES NOT SHOW.  A small p-value says that the tables differ by more than relabelling explains; it does not say by how
much.  With ``n`` large the test rejects at differences far too small to matter for any use of the synthetic table, so read ``d2``
itself, and the ``d2`` and p-value against a HELD-OUT split beside it: a synthetic table that is as far from the training split as the
held-out split is has done what can be asked.  A large p-value at small ``n`` shows little either.

``permutation_labels`` is torch plumbing on the host with no performance claim: one ``torch.randperm`` draw per labelling from a
``torch.Generator`` seeded with ``seed`` (so the labels of labelling ``r`` do not depend on the chunk in which they are made), the
first ``n_y`` entries being the rows that carry the 1.  The words are tile-major: bit ``p`` of ``labels[tile, r]`` is row ``32 tile +
p``.  It is a pure function of its arguments.

``label_sums`` is the kernel call: ``z`` a 2-D CUDA tensor ``(m, d)``, float32 or int32, with unit column stride and any row stride
``>= d`` (1-D: ``d = 1``); ``labels`` uint32, contiguous, ``(ceil(m / 32), R)`` on the same device, ``R`` within
``d3p_pair_label_sums_max_labellings()``; bits of rows ``>= m`` are ignored.  ``row_sum`` defaults to ``fidelity.pair_stats(z, z,
True)["sum"]``; ``total = torch.sum(row_sum)`` (no bit promise).  int32 values beyond ``2^24`` in magnitude are a ``ValueError`` (this
one check reads the table, so it runs on the device, after every other).  A NaN or infinite element anywhere in ``z`` makes every
``s11`` NaN.  The workspace is allocated with ``torch.empty``.  Every other host check runs before the device is touched; there is no
CPU fallback.
"""
from typing import NamedTuple, Tuple

import torch

from . import _lib
from . import fidelity as FD
from ._lib import check, ptr, stream_ptr
from .energy import INT_EXACT

__all__ = ["permutation_labels", "label_sums", "energy_test", "LabelSums", "EnergyTest", "INT_EXACT"]

_TILE = 32
_LABEL_CHUNK = 64          # labellings made at once by permutation_labels (bounds the temporary; changes no output)
_QUANTILES = (0.5, 0.95, 0.99)


class LabelSums(NamedTuple):
    s11: torch.Tensor      # (R,) float64: sum_{i,j} g_i g_j D_ij
    s1t: torch.Tensor      # (R,) float64: sum_i g_i row_sum[i]
    n1: torch.Tensor       # (R,) int64: the rows that carry the 1
    total: torch.Tensor    # 0-d float64: sum_i row_sum[i]
    m: int


class EnergyTest(NamedTuple):
    d2: torch.Tensor               # 0-d float64: the V-statistic energy distance of the identity labelling
    statistic: torch.Tensor        # 0-d float64: n_x n_y / (n_x + n_y) d2
    p_value: float                 # (1 + n_ge) / (n_perm + 1)
    n_perm: int
    null_mean: torch.Tensor        # 0-d float64: the mean statistic of the relabellings
    null_quantiles: Tuple[float, ...]   # its 0.5 / 0.95 / 0.99 quantiles
    n_ge: int                      # #{r >= 1 : statistic_r >= statistic_0}, a tie counting
    n_x: int
    n_y: int
    dim: int


def _count(v, name, what, least):
    if isinstance(v, bool) or not isinstance(v, int) or v < least:
        raise ValueError(f"{what}: {name} must be an int >= {least}, got {v!r}")
    return v


def permutation_labels(n_x, n_y, n_perm, seed=0, device=None, _chunk=_LABEL_CHUNK):
    """The label words of the identity labelling (column 0: rows ``>= n_x`` set) and of ``n_perm`` uniform random subsets of ``n_y`` of
    the ``n_x + n_y`` pooled rows: a ``(ceil(m / 32), n_perm + 1)`` uint32 tensor on ``device`` (module docstring).  One generator draw per
    labelling: the output does not depend on the chunk size (``_chunk``, the labellings packed at once: a test aid)."""
    what = "permutation_labels"
    n_x, n_y, n_perm = _count(n_x, "n_x", what, 1), _count(n_y, "n_y", what, 1), _count(n_perm, "n_perm", what, 1)
    _count(seed, "seed", what, 0)
    _count(_chunk, "_chunk", what, 1)
    m = n_x + n_y
    if m > FD._MAX_ROWS:
        raise ValueError(f"{what}: {m} pooled rows; at most {FD._MAX_ROWS}")
    tiles = -(-m // _TILE)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    weights = torch.tensor([1 << p for p in range(_TILE)], dtype=torch.int64)
    out = torch.empty((tiles, n_perm + 1), dtype=torch.int64)
    for lo in range(0, n_perm + 1, _chunk):
        hi = min(lo + _chunk, n_perm + 1)
        bits = torch.zeros((hi - lo, tiles * _TILE), dtype=torch.int64)
        for r in range(lo, hi):
            if r == 0:
                bits[0, n_x:m] = 1
            else:
                bits[r - lo, torch.randperm(m, generator=gen)[:n_y]] = 1
        out[:, lo:hi] = (bits.view(hi - lo, tiles, _TILE) * weights).sum(dim=2).t()
    words = torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32).contiguous().view(torch.uint32)
    return words if device is None else words.to(device)


def _check_labels(labels, m, what):
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint32 or labels.dim() != 2:
        raise ValueError(f"{what}: labels: a 2-D uint32 tensor (ceil(m / 32), R) is required")
    tiles = -(-m // _TILE)
    if int(labels.shape[0]) != tiles:
        raise ValueError(f"{what}: labels has {int(labels.shape[0])} rows of words; {m} rows of z need {tiles}")
    R = int(labels.shape[1])
    if R < 1:
        raise ValueError(f"{what}: labels: at least one labelling")
    if not labels.is_contiguous():
        raise ValueError(f"{what}: labels must be contiguous")
    cap = int(_lib.load().d3p_pair_label_sums_max_labellings())
    if R > cap:
        raise ValueError(f"{what}: {R} labellings; at most {cap} in one call")
    return R


def _sums(z, dz, labels, R, row_sum):
    """One call of d3p_pair_label_sums on checked arguments."""
    m, d, ld = dz
    lib = _lib.load()
    dev = z.device
    s11 = torch.empty(R, dtype=torch.float64, device=dev)
    s1t = torch.empty(R, dtype=torch.float64, device=dev)
    n1 = torch.empty(R, dtype=torch.int32, device=dev)
    need = int(lib.d3p_pair_label_sums_workspace(m, d, R))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    check(lib.d3p_pair_label_sums(stream_ptr(), ptr(z), 0 if z.dtype == torch.float32 else 1, ld, m, d, R, ptr(labels), ptr(row_sum),
                                  ptr(s11), ptr(s1t), ptr(n1), ptr(ws), int(ws.numel())))
    return s11, s1t, n1.to(torch.int64) & 0xFFFFFFFF


def label_sums(z, labels, row_sum=None):
    """``s11``, ``s1t`` and ``n1`` of every labelling in ``labels`` over the pooled table ``z`` (module docstring): a ``LabelSums`` on
    the table's device.  ``row_sum`` defaults to ``fidelity.pair_stats(z, z, True)["sum"]``."""
    what = "label_sums"
    dz = FD._check_table(z, "z", what)
    R = _check_labels(labels, dz[0], what)
    if row_sum is not None:
        if not isinstance(row_sum, torch.Tensor) or row_sum.dtype != torch.float64 or row_sum.dim() != 1 or int(row_sum.shape[0]) != dz[0] \
                or not row_sum.is_contiguous():
            raise ValueError(f"{what}: row_sum: a contiguous float64 tensor ({dz[0]},) is required")
    FD._check_devices((("z", z),), what)
    if labels.device != z.device or (row_sum is not None and row_sum.device != z.device):
        raise ValueError(f"{what}: z, labels and row_sum lie on different devices")
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(z.device):
        FD._check_exact((("z", z),), what)
        if row_sum is None:
            row_sum = FD.pair_stats(z, z, True)["sum"]
        s11, s1t, n1 = _sums(z, dz, labels, R, row_sum)
        return LabelSums(s11, s1t, n1, torch.sum(row_sum), dz[0])


def _statistics(s11, s1t, n1, total, m):
    """(d2, statistic) per labelling from the sums, in float64 (module docstring)."""
    n1 = n1.to(torch.float64)
    n0 = float(m) - n1
    s10 = s1t - s11
    s00 = total - 2.0 * s10 - s11
    d2 = 2.0 * s10 / (n1 * n0) - s11 / (n1 * n1) - s00 / (n0 * n0)
    return d2, n1 * n0 / (n1 + n0) * d2


def _p_value(stat):
    """(n_ge, p) of a vector of statistics whose entry 0 is the observed one: a tie counts."""
    n_ge = int((stat[1:] >= stat[0]).sum())
    return n_ge, (1 + n_ge) / int(stat.shape[0])


def energy_test(x, y, n_perm=999, seed=0):
    """The permutation test of the energy distance of the tables ``x`` and ``y`` (module docstring): an ``EnergyTest``.  These are
    functions of the PRIVATE tables and are not covered by the accountant."""
    what = "energy_test"
    dx, dy = FD._check_pair(x, y, ("x", "y"), what)
    n_perm = _count(n_perm, "n_perm", what, 1)
    _count(seed, "seed", what, 0)
    nx, ny, d = dx[0], dy[0], dx[1]
    m = nx + ny
    if m > FD._MAX_ROWS:
        raise ValueError(f"{what}: {m} pooled rows; at most {FD._MAX_ROWS}")
    FD._check_devices((("x", x), ("y", y)), what)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(x.device):
        FD._check_exact((("x", x), ("y", y)), what)
        z = torch.cat([x.reshape(nx, d), y.reshape(ny, d)], dim=0).contiguous()
        dz = (m, d, d)
        labels = permutation_labels(nx, ny, n_perm, seed, device=z.device)
        row_sum = FD.pair_stats(z, z, True)["sum"]
        cap = int(_lib.load().d3p_pair_label_sums_max_labellings())
        parts = []
        for lo in range(0, n_perm + 1, cap):      # (above the cap: chunks of labellings, the row sums reused)
            part = labels[:, lo:lo + cap].contiguous()
            parts.append(_sums(z, dz, part, int(part.shape[1]), row_sum))
        s11, s1t, n1 = (torch.cat([p[k] for p in parts]) for k in range(3))
        d2, stat = _statistics(s11, s1t, n1, torch.sum(row_sum), m)
        n_ge, p = _p_value(stat)
        null = stat[1:]
        quant = torch.quantile(null, torch.tensor(_QUANTILES, dtype=torch.float64, device=null.device))
        return EnergyTest(d2[0], stat[0], p, n_perm, null.mean(), tuple(float(v) for v in quant), n_ge, nx, ny, d)
