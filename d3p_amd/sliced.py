"""The sliced Wasserstein distance of a synthetic table against a real one: both tables projected onto random
directions on the matrix cores, every projection sorted over ALL rows, the exact one-dimensional Wasserstein distances per direction,
and their average -- a multivariate two-sample distance that is a metric, sees beyond second moments and costs ``O(n log n)``.

    random_directions(d, n_dirs, seed=0, scale=None, device=None)  -> (d, n_dirs) float32
    project(x, theta, shift=None)                                  -> (n, L) float32
    w2_distance(sa, sb)                                            -> (d,) float64 of two sort_columns results
    sliced_wasserstein(real, synthetic, n_dirs=128, seed=0, scale="std", holdout=None, slab_bytes=1 << 30)
                                                                   -> SlicedWasserstein

PRIVACY.  Every number here is computed from the PRIVATE table, without noise.  Releasing a distance or a correlation, or choosing a
model by looking at one, is NOT covered by the accountant (``DPSVI.get_epsilon``): the accountant covers the noised steps of training
and nothing else.  The functions are a diagnostic for the person who holds the data.

``random_directions`` is a host job of ``d * n_dirs`` numbers: float64 normals from a ``torch.Generator`` on the CPU, direction by
direction (so direction ``l`` depends on ``(seed, d, l)`` alone and a slab of directions reproduces it), each direction normalised in
float64, multiplied by ``scale`` (a ``(d,)`` vector: the kernel knows nothing of it), rounded ONCE to float32 and moved to ``device``.

``project`` is the kernel call (``d3p_project_rows``, ``d3p_amd/csrc/d3p_sliced.hip``): ``x`` a table as ``univariate.sort_columns``
takes it (int32: exact up to ``INT_EXACT = 2^24``, which ``sliced_wasserstein`` checks and ``project`` leaves to the caller), ``theta``
a 2-D float32 tensor ``(d, L)`` with unit column stride, ``shift`` a contiguous ``(d,)`` float32 tensor or None:
``p[i, l] = sum_c fl32(x[i, c] - shift[c]) theta[c, l]`` in one fixed order, within the bound the kernel's header states; a NaN in a
row gives NaN in all its projections.  The result is the table ``sort_columns`` reads.

``w2_distance`` is ``d3p_column_w2_distance`` on two ``sort_columns`` results ``(d, n_a)`` and ``(d, n_b)``: the exact squared
2-Wasserstein distance of the empirical distributions per column, ``integral (F_a^-1 - F_b^-1)^2`` over the ``n_a n_b`` levels, in
float64 in one fixed order; NaN for a column that holds a NaN or an infinity in either table.

``sliced_wasserstein`` compares ``synthetic`` with ``real``.  ``scale="std"`` divides every column by the real table's standard
deviation (``covariance.column_moments``, ``ddof = 1``; a constant column, and every column of a one-row table, gets 0), ``None``
leaves the units alone, a ``(d,)`` tensor is used as given.  The shift of BOTH tables is the real table's float32 column mean: W_p is
translation invariant, so this costs nothing and keeps the digits of a column such as a year.  The directions are taken in slabs, so
that the projections of the two tables stay within ``slab_bytes``; per slab two ``project`` calls, two column sorts, the KS /
Wasserstein-1 kernel and ``w2_distance``.  The slab width changes no bit.

    sw1, sw2              the mean of ``w1`` and the root of the mean of ``w2sq`` over the directions
    max_w1, max_w2        the max-sliced distances (``max_w2`` the root of the largest ``w2sq``), ``max_w1_at``, ``max_w2_at`` their directions
    w1, w2sq, ks          (n_dirs,) float64 per direction
    floor                 with a ``holdout``: the same for holdout against real (its own ``floor`` None)

The Monte-Carlo error of the estimate over the directions is the user's to judge from the per-direction vectors: under ``scale`` the
terms are not identically distributed, and no standard error is computed of a thing that is not i.i.d.

Every host check runs before the device is touched; there is no CPU fallback.
"""
from typing import NamedTuple, Optional

import torch

from . import _lib
from . import _tables as T
from . import covariance as CV
from . import univariate as UV
from ._lib import check, ptr, stream_ptr
from ._tables import INT_EXACT

__all__ = ["random_directions", "project", "w2_distance", "sliced_wasserstein", "SlicedWasserstein", "INT_EXACT"]


class SlicedWasserstein(NamedTuple):
    sw1: float
    sw2: float
    max_w1: float
    max_w1_at: int
    max_w2: float
    max_w2_at: int
    w1: torch.Tensor       # (n_dirs,) float64
    w2sq: torch.Tensor     # (n_dirs,) float64
    ks: torch.Tensor       # (n_dirs,) float64
    n_dirs: int
    n_real: int
    n_synthetic: int
    dim: int
    seed: int
    floor: Optional["SlicedWasserstein"]


def _check_scale(scale, d, what):
    if scale is None:
        return None
    if not isinstance(scale, torch.Tensor) or scale.dim() != 1 or int(scale.shape[0]) != d or not scale.dtype.is_floating_point:
        raise ValueError(f"{what}: scale must be None or a floating-point tensor of shape ({d},)")
    return scale


def random_directions(d, n_dirs, seed=0, scale=None, device=None):
    """``n_dirs`` random unit directions of ``d`` columns, times ``scale``, as a ``(d, n_dirs)`` float32 tensor (module docstring)."""
    what = "random_directions"
    T.check_int(d, "d", what, 1)
    T.check_int(n_dirs, "n_dirs", what, 1)
    T.check_int(seed, "seed", what, 0)
    scale = _check_scale(scale, d, what)
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    z = torch.stack([torch.randn(d, generator=g, dtype=torch.float64) for _ in range(n_dirs)], dim=1)
    z = z / z.norm(dim=0)
    if scale is not None:
        z = z * scale.detach().to(device="cpu", dtype=torch.float64)[:, None]
    theta = z.to(torch.float32)
    return theta if device is None else theta.to(device)


def _check_theta(theta, shift, d, what):
    if not isinstance(theta, torch.Tensor) or theta.dim() != 2 or theta.dtype != torch.float32:
        raise ValueError(f"{what}: theta: a 2-D float32 CUDA tensor (d, n_dirs) is required")
    if int(theta.shape[0]) != d or int(theta.shape[1]) < 1:
        raise ValueError(f"{what}: theta has shape {tuple(theta.shape)}: ({d}, n_dirs >= 1) is required")
    L = int(theta.shape[1])
    if L > 1 and theta.stride(1) != 1:
        raise ValueError(f"{what}: theta: the directions must have unit stride (the rows may be strided)")
    ld_t = T.check_row_stride(theta, "theta", what)
    T.check_column_vector(shift, "shift", d, what)
    return L, ld_t


def _project(x, dx, theta, dt, shift):
    """One call of d3p_project_rows on checked arguments: the (n, L) float32 projections."""
    n, d, ld = dx
    L, ld_t = dt
    p = torch.empty((n, L), dtype=torch.float32, device=x.device)
    check(_lib.load().d3p_project_rows(stream_ptr(), ptr(x), T.dtype_code(x), ld, n, d, ptr(theta), ld_t, L, ptr(shift), ptr(p), L))
    return p


def project(x, theta, shift=None):
    """The rows of ``x``, less ``shift``, projected onto the columns of ``theta`` (module docstring): ``(n, L)`` float32."""
    what = "project"
    dx = T.check_rows(T.check_table(x, "x", what), "x", what, False)
    dt = _check_theta(theta, shift, dx[1], what)
    with T.on_device((("x", x), ("theta", theta), ("shift", shift)), what):
        return _project(x, dx, theta, dt, shift)


def _check_sorted(s, name, what):
    if not isinstance(s, torch.Tensor) or s.dim() != 2 or s.dtype not in (torch.float32, torch.int32):
        raise ValueError(f"{what}: {name}: a 2-D float32 or int32 CUDA tensor (d, n), as sort_columns returns it, is required")
    d, n = int(s.shape[0]), int(s.shape[1])
    if d < 1 or n < 1:
        raise ValueError(f"{what}: {name}: at least one column and one value per column")
    if n > T.MAX_ROWS_SORTED:
        raise ValueError(f"{what}: {name}: {n} values per column; at most 2^31 - 1")
    if n > 1 and s.stride(1) != 1:
        raise ValueError(f"{what}: {name}: the values of a column must have unit stride")
    ld = int(s.stride(0)) if d > 1 else n
    if ld < n:
        raise ValueError(f"{what}: {name}: the columns of the tensor overlap (strides {tuple(s.stride())})")
    return d, n, ld


def _w2(sa, da, sb, db):
    """One call of d3p_column_w2_distance on two checked sorted tables."""
    (d, n_a, ld_a), (_, n_b, ld_b) = da, db
    lib = _lib.load()
    out = torch.empty(d, dtype=torch.float64, device=sa.device)
    ws = torch.empty(int(lib.d3p_column_w2_distance_workspace(n_a, n_b, d)), dtype=torch.uint8, device=sa.device)
    check(lib.d3p_column_w2_distance(stream_ptr(), ptr(sa), ld_a, n_a, ptr(sb), ld_b, n_b, T.dtype_code(sa), d, ptr(out), ptr(ws),
                                     int(ws.numel())))
    return out


def w2_distance(sa, sb):
    """The squared 2-Wasserstein distance per column of two ``sort_columns`` results (module docstring): ``(d,)`` float64.  These are
    functions of the PRIVATE tables and are not covered by the accountant."""
    what = "w2_distance"
    da, db = _check_sorted(sa, "sa", what), _check_sorted(sb, "sb", what)
    T.check_match(sa, sb, da[0], db[0], ("sa", "sb"), what)
    with T.on_device((("sa", sa), ("sb", sb)), what):
        return _w2(sa, da, sb, db)


def _distance(a, da, b, db, theta, shift, width, seed):
    """SlicedWasserstein (floor None) of two checked tables under the directions theta, taken in slabs of `width`."""
    L = int(theta.shape[1])
    w1, w2sq, ks = [], [], []
    for lo in range(0, L, width):
        th = theta[:, lo:lo + width]
        w = int(th.shape[1])
        sorted_ = []
        for t, dt in ((a, da), (b, db)):
            p = _project(t, dt, th, (w, L), shift)
            sorted_.append(UV._sort(p, (dt[0], w, w), False)[0])
            del p
        dist = UV._cdf(sorted_[0], sorted_[1])
        w1.append(dist.w1)
        ks.append(dist.ks)
        w2sq.append(_w2(sorted_[0], (w, da[0], da[0]), sorted_[1], (w, db[0], db[0])))
    w1, w2sq, ks = torch.cat(w1), torch.cat(w2sq), torch.cat(ks)
    m1, m2 = torch.max(w1, 0), torch.max(w2sq, 0)
    return SlicedWasserstein(float(w1.mean()), float(w2sq.mean().sqrt()), float(m1.values), int(m1.indices), float(m2.values.sqrt()),
                             int(m2.indices), w1, w2sq, ks, L, da[0], db[0], da[1], seed, None)


def sliced_wasserstein(real, synthetic, n_dirs=128, seed=0, scale="std", holdout=None, slab_bytes=1 << 30):
    """The sliced 1- and 2-Wasserstein distances of ``synthetic`` against ``real`` over ``n_dirs`` random directions -- and, with a
    ``holdout``, the noise floor that the holdout scores against ``real`` (module docstring): a ``SlicedWasserstein``.  These are
    functions of the PRIVATE tables and are not covered by the accountant."""
    what = "sliced_wasserstein"
    tables = T.check_group(real, synthetic, holdout, ("real", "synthetic", "holdout"), what)
    dr = tables[0][2]
    for name, _, dx in tables:
        T.check_rows(dx, name, what, False)
    T.check_int(n_dirs, "n_dirs", what, 1)
    T.check_int(seed, "seed", what, 0)
    T.check_int(slab_bytes, "slab_bytes", what, 1)
    if not (scale is None or (isinstance(scale, str) and scale == "std")):
        _check_scale(scale, dr[1], what)
    with T.on_device(tables, what, exact=tables):
        shift, inv_std = CV.standardise(real, dr)
        if isinstance(scale, str):
            scale = inv_std
        theta = random_directions(dr[1], n_dirs, seed, scale, real.device)
        rep = []
        for _, t, dx in tables[1:]:
            width = max(1, min(n_dirs, slab_bytes // (4 * (dr[0] + dx[0]))))
            rep.append(_distance(real, dr, t, dx, theta, shift, width, seed))
        return rep[0] if holdout is None else rep[0]._replace(floor=rep[1])
