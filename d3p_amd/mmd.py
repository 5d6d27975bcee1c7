"""The maximum mean discrepancy of a synthetic table against a real one with a Gaussian kernel over a ladder of bandwidths (Gretton et
al. 2012): per-row kernel sums from a Gram walk on the matrix cores, without the ``n_a x n_b`` matrix.

    kernel_sums(a, b, gamma0, n_bandwidths=1, shift=None, scale=None, exclude_diagonal=False)  -> (B, n_a) float64
    mmd(x, y, bandwidth="median", n_bandwidths=5, scale="std")                                 -> MMD

PRIVACY.  Every number here is computed from the PRIVATE table, without noise.  Releasing a discrepancy or a witness value, or choosing
a model by looking at one, is NOT covered by the accountant (``DPSVI.get_epsilon``): the accountant covers the noised steps of training
and nothing else.  The functions are a diagnostic for the person who holds the data.

``kernel_sums`` is the kernel call (``d3p_kernel_sums``, ``d3p_amd/csrc/d3p_mmd.hip``).  ``a`` and ``b`` are tables as
``fidelity.pair_stats`` takes them (one dtype, float32 or int32 -- exact up to ``INT_EXACT = 2^24`` --, one device, unit column stride, any
row stride ``>= d``, at most ``2^31 - 1`` rows); ``shift`` and ``scale`` are contiguous ``(d,)`` float32 tensors or None; ``gamma0`` a
finite float ``> 0`` (it is rounded to float32).  With ``t = fl32(fl32(x - shift) * scale)`` and ``q_ij = |ta_i|^2 + |tb_j|^2 - 2 ta_i .
tb_j`` from the float32 Gram product, clamped at 0,

    out[b, i] = sum_j exp2(-gamma0 * 2^b * q_ij)        b = 0 .. n_bandwidths - 1 <= 7

over all ``j`` -- without ``j == i`` when ``exclude_diagonal`` is set, which needs ``n_a == n_b`` --, in float64 in one fixed order:
one exponential and ``b`` squarings a pair.  A row without an admissible ``j`` gets 0; a NaN or infinite element in row ``i`` of ``a``
makes that row NaN for every ``b`` and one anywhere in ``b`` every row.  The Gram form is safe HERE and not for a nearest record: the
kernel is flat at ``q = 0``, so an absolute error of ``q`` costs ``gamma k`` times it -- on tables centred by ``shift`` a few ``d u`` of
``k``; the kernel's header derives the bound.  Pass a ``shift`` near the column means: without one a table far from the origin loses the
digits of ``q``.  Repeated calls give equal bits.

``mmd`` compares ``y`` with ``x`` under ``k(u, v) = exp(-|u - v|^2 / (2 sigma^2))`` in the space ``t``: the shift is the float32 column
mean of ``x``, the scale ``1 / std`` of ``x`` (``covariance.column_moments``, ``ddof = 1``; a constant column, and every column of a
one-row table, gets 0) under ``scale="std"`` and none under ``None``.  ``bandwidth="median"`` centres the ladder on the median of the
squared distances in that space between the pairs of the pooled, evenly strided subsample of at most 1024 rows of each table (a cold
path in torch, float64); a float is the centre ``sigma^2`` itself.  The ``B = n_bandwidths`` bandwidths are ``sigma2[b] = centre *
2^((B - 1) / 2 - b)`` and ``gamma0 = 1 / (2 ln 2 sigma2[0])``.  Four walks -- ``(x, y)``, ``(y, x)``, ``(x, x)`` and ``(y, y)`` without
their diagonals -- give per bandwidth

    kxy, kxx, kyy         the means of k over n_x n_y, n_x^2 and n_y^2 pairs; the diagonals enter kxx and kyy as the exact n
    mmd2                  kxx + kyy - 2 kxy, the V-statistic (>= 0 up to rounding)
    mmd2_unbiased         with n (n - 1) pairs and no diagonal in the within-table means (NaN when a table has one row)
    sigma2                the bandwidths as sigma^2
    witness_x, witness_y  f(z) = mean_j k(z, x_j) - mean_j k(z, y_j) at the rows of x, (B, n_x), and of y, (B, n_y): where it is far
                          from 0 the tables disagree (positive: x is denser there)

all ``(B,)`` float64 but the witnesses.  The witness at the rows of ``y`` needs the sums of ``k(y_i, x_j)`` over ``j``, which the rows of
the ``(x, y)`` walk do not hold: that is the fourth walk.  The closing totals are ``torch.sum`` in float64 and carry no bit promise.
Equal tables give ``mmd2`` within the kernel's bound of 0, not exactly 0: the ``(x, y)`` walk computes its diagonal, ``k_ii =
exp2(-gamma0 q_ii)`` with ``q_ii`` a rounding residue, where the within-table means hold the exact 1.

Every other host check runs before the device is touched; there is no CPU fallback.
"""
import math
from typing import NamedTuple

import torch

from . import _lib
from . import _tables as T
from . import covariance as CV
from ._lib import check, ptr, stream_ptr
from ._tables import INT_EXACT

__all__ = ["kernel_sums", "mmd", "MMD", "INT_EXACT"]

MAX_BANDWIDTHS = 8


class MMD(NamedTuple):
    mmd2: torch.Tensor            # (B,) float64: kxx + kyy - 2 kxy, V-statistic
    mmd2_unbiased: torch.Tensor   # (B,) with n (n - 1) in kxx and kyy and no diagonal (NaN when a table has one row)
    kxy: torch.Tensor             # (B,)
    kxx: torch.Tensor             # (B,) over n_x^2 pairs, the diagonal's n_x included
    kyy: torch.Tensor             # (B,)
    sigma2: torch.Tensor          # (B,) the bandwidths as sigma^2, descending
    witness_x: torch.Tensor       # (B, n_x)
    witness_y: torch.Tensor       # (B, n_y)
    n_x: int
    n_y: int
    dim: int


def _check_bandwidths(n_bandwidths, what):
    if isinstance(n_bandwidths, bool) or not isinstance(n_bandwidths, int) or not 1 <= n_bandwidths <= MAX_BANDWIDTHS:
        raise ValueError(f"{what}: n_bandwidths must be an int in 1 .. {MAX_BANDWIDTHS}, got {n_bandwidths!r}")
    return n_bandwidths


def _sums(a, da, b, db, gamma0, n_bandwidths, shift, scale, exclude):
    """One call of d3p_kernel_sums on checked tables: the (B, n_a) float64 sums."""
    (na, d, a_ld), (nb, _, b_ld) = da, db
    lib = _lib.load()
    out = torch.empty((n_bandwidths, na), dtype=torch.float64, device=a.device)
    ws = torch.empty(int(lib.d3p_kernel_sums_workspace(na, nb, n_bandwidths)), dtype=torch.uint8, device=a.device)
    check(lib.d3p_kernel_sums(stream_ptr(), ptr(a), ptr(b), T.dtype_code(a), a_ld, b_ld, na, nb, d, ptr(shift), ptr(scale),
                              gamma0, n_bandwidths, 1 if exclude else 0, ptr(out), ptr(ws), int(ws.numel())))
    return out


def kernel_sums(a, b, gamma0, n_bandwidths=1, shift=None, scale=None, exclude_diagonal=False):
    """Per row of ``a`` and per bandwidth the float64 sum of ``exp2(-gamma0 2^b q)`` over the rows of ``b`` (module docstring): ``(B,
    n_a)`` on the tables' device.  ``exclude_diagonal=True`` leaves out ``j == i`` (a table against itself: ``n_a == n_b``)."""
    what = "kernel_sums"
    da, db = T.check_pair(a, b, ("a", "b"), what)
    T.check_rows(da, "a", what, False)
    T.check_rows(db, "b", what, False)
    gamma0 = T.check_positive(gamma0, "gamma0", what)
    _check_bandwidths(n_bandwidths, what)
    T.check_column_vector(shift, "shift", da[1], what)
    T.check_column_vector(scale, "scale", da[1], what)
    exclude = T.check_diagonal(exclude_diagonal, da, db, what)
    tables = (("a", a), ("b", b))
    with T.on_device(tables + (("shift", shift), ("scale", scale)), what, exact=tables):
        return _sums(a, da, b, db, gamma0, n_bandwidths, shift, scale, exclude)


def _ladder(centre, n_bandwidths):
    """(sigma2 as a list, gamma0) of the ladder centred on ``centre``: sigma2[b] = centre 2^((B - 1) / 2 - b)."""
    sigma2 = [centre * 2.0 ** (0.5 * (n_bandwidths - 1) - b) for b in range(n_bandwidths)]
    return sigma2, 1.0 / (2.0 * math.log(2.0) * sigma2[0])


def _closing(sxy, syx, sxx, syy, sigma2, d):
    """MMD from the per-row sums of the four walks, (B, n) float64 each; sxx and syy without their diagonals."""
    nx, ny = int(sxy.shape[1]), int(syx.shape[1])
    txy, txx, tyy = torch.sum(sxy, dim=1), torch.sum(sxx, dim=1), torch.sum(syy, dim=1)
    kxy, kxx, kyy = txy / (nx * ny), (txx + nx) / (nx * nx), (tyy + ny) / (ny * ny)
    ux = txx / torch.tensor(float(nx * (nx - 1)), dtype=torch.float64, device=txx.device)      # (0 / 0 = NaN at one row)
    uy = tyy / torch.tensor(float(ny * (ny - 1)), dtype=torch.float64, device=tyy.device)
    witness_x = (sxx + 1.0) / nx - sxy / ny
    witness_y = syx / nx - (syy + 1.0) / ny
    return MMD(kxx + kyy - 2.0 * kxy, ux + uy - 2.0 * kxy, kxy, kxx, kyy, torch.tensor(sigma2, dtype=torch.float64, device=sxy.device),
               witness_x, witness_y, nx, ny, d)


def mmd(x, y, bandwidth="median", n_bandwidths=5, scale="std"):
    """The squared maximum mean discrepancy of ``y`` against ``x`` under Gaussian kernels of ``n_bandwidths`` bandwidths, with the
    witness function at every row (module docstring): an ``MMD``.  These are functions of the PRIVATE tables and are not covered by the
    accountant."""
    what = "mmd"
    dx, dy = T.check_pair(x, y, ("x", "y"), what)
    T.check_rows(dx, "x", what, False)
    T.check_rows(dy, "y", what, False)
    if not (isinstance(bandwidth, str) and bandwidth == "median"):
        if isinstance(bandwidth, str):
            raise ValueError(f"{what}: bandwidth must be 'median' or a finite number > 0 (the centre sigma^2), got {bandwidth!r}")
        bandwidth = T.check_positive(bandwidth, "bandwidth", what)
    _check_bandwidths(n_bandwidths, what)
    if not (scale is None or (isinstance(scale, str) and scale == "std")):
        raise ValueError(f"{what}: scale must be 'std' or None, got {scale!r}")
    tables = (("x", x), ("y", y))
    with T.on_device(tables, what, exact=tables):
        shift, inv_std = CV.standardise(x, dx)
        if scale is not None:
            scale = inv_std.to(torch.float32)
        if isinstance(bandwidth, str):
            bandwidth = T.median_q(x, y, shift, scale)
            if not (bandwidth > 0 and math.isfinite(bandwidth)):
                raise ValueError(f"{what}: the median squared distance of the subsample is {bandwidth}: pass a bandwidth")
        sigma2, gamma0 = _ladder(bandwidth, n_bandwidths)
        walks = [_sums(a, da, b, db, gamma0, n_bandwidths, shift, scale, excl)
                 for a, da, b, db, excl in ((x, dx, y, dy, False), (y, dy, x, dx, False), (x, dx, x, dx, True), (y, dy, y, dy, True))]
        return _closing(*walks, sigma2, dx[1])
