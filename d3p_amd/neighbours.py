"""k nearest neighbours of two tables and the k-NN-ball fidelity of a synthetic table: improved precision and recall, density and
coverage, and the authenticity score.

    knn(a, b, k, exclude_diagonal=False, radius_sq=None)
        -> {"distance": (na, k) float32, "sq": (na, k) float32, "index": (na, k) int64 (-1: none)[, "count": (na,) int64 (-1: flagged)]}
    kth_neighbour(x, k)          -> {"distance": (n,), "sq": (n,)}: the k-th nearest OTHER row of x
    ball_counts(a, b, radius_sq) -> (na,) int64
    prdc(real, synthetic, k=5, holdout=None) -> PRDC(precision, recall, density, coverage, authenticity, k, n_real, n_synthetic, dim, floor)

PRIVACY.  Every number here is computed from the PRIVATE table, without noise.  Releasing a score, or choosing a model by looking at
it, is NOT covered by the accountant (``DPSVI.get_epsilon``): the accountant covers the noised steps of training and nothing else.  The
functions are a diagnostic for the person who holds the data.

``d3p_amd.fidelity`` answers whether two tables have one distribution and whether records were copied; one number of its kind mixes
two failures of a generator that call for different cures.  Poor QUALITY: synthetic rows lie outside the real data's support.  Poor
COVERAGE: modes of the real table are never produced.  The k-NN-ball family tells them apart, and all of it reduces the distance of
every row to its k-th nearest neighbour inside its own table and the membership of rows in the balls of that radius -- one ``O(n_a n_b
d)`` walk over the pairs of two tables (``d3p_pair_knn``, ``d3p_amd/csrc/d3p_pair_knn.hip``) that carries an exact per-row top-k
selection and the ball counts along, without the ``n_a x n_b`` matrix.

``knn`` is the model-free reduction.  ``a`` and ``b`` are tables as ``fidelity.pair_stats`` takes them: 2-D CUDA tensors ``(n, d)`` of
one dtype, float32 or int32, on one device, with unit column stride and any row stride ``>= d``; a 1-D tensor is ``d = 1``.  ``sq`` is
the float32 squared distance of the kernel's header (``t = fl32(a_c - b_c)``, an fmaf chain over the columns), ``distance`` its
correctly rounded root.  Per row ``i`` over all ``j < n_b`` -- without ``j == i`` when ``exclude_diagonal`` is set, which needs ``n_a ==
n_b`` -- the ``k`` pairs with the smallest ``(sq, j)`` in ascending order: among equal ``sq`` the smallest ``j`` first.  ``1 <= k <=
max_k()`` (16).  Places that fewer than ``k`` admissible rows leave hold ``+inf, +inf, -1``.  ``radius_sq`` is a float32 CUDA tensor
``(n_b,)`` of SQUARED radii, one per row of ``b``; with it ``count[i] = #{j : sq(i, j) < radius_sq[j]}``, strictly (as the ``prdc``
package compares) and by IEEE: a NaN radius contains nothing, ``+inf`` every finite ``sq``.  A NaN or infinite element in row ``i`` of
``a`` makes that row ``NaN, NaN, -1`` with count ``-1``, and one anywhere in ``b`` every row.  Everything selected or counted is an
integer, so the outputs are deterministic to the bit and depend on that row, ``b``, the radii and the flag alone; at ``k = 1``
``distance`` and ``index`` are ``pair_stats``' ``min`` and ``argmin``.  int32 values beyond ``2^24`` in magnitude are a ``ValueError``
(this one check reads the tables, so it runs on the device, after every other).  The workspace is allocated with ``torch.empty``.

``prdc`` makes four walks, with ``R`` = real, ``S`` = synthetic:

    RR = knn(R, R, k, True)      SS = knn(S, S, k, True)
    SR = knn(S, R, 1, radius_sq=RR.sq[:, k-1])       RS = knn(R, S, 1, radius_sq=SS.sq[:, k-1])

and compares float32 squared distances throughout:

    precision    = mean_j 1[SR.count[j] > 0]              a synthetic row lies in some real row's k-NN ball (Kynkaanniemi et al. 2019)
    recall       = mean_i 1[RS.count[i] > 0]              a real row lies in some synthetic row's ball
    density      = sum_j SR.count[j] / (k n_S)            how many real balls hold a synthetic row (Naeem et al. 2020); may exceed 1
    coverage     = mean_i 1[RS.sq[i, 0] < RR.sq[i, k-1]]  a real row's own ball holds a synthetic row
    authenticity = mean_j 1[SR.sq[j, 0] > RR.sq[SR.index[j, 0], 0]]     (Alaa et al. 2022) the synthetic row is farther from its nearest
                   real row than that real row is from its own nearest real neighbour: not a noisy copy

``floor`` is ``prdc(real, holdout, k)`` without a floor of its own -- what a fresh sample of the real distribution scores, the level a
perfect generator reaches -- and ``None`` without a holdout.  Fewer than ``k + 1`` rows in a table is a ``ValueError``, and so is a
NaN or infinite element in one (found on the device, from the flagged rows of the walks: no share is taken over them).

Every other host check runs before the device is touched; there is no CPU fallback.
"""
from typing import NamedTuple, Optional

import torch

from . import _lib
from . import _tables as T
from ._lib import check, ptr, stream_ptr
from ._tables import INT_EXACT

__all__ = ["knn", "kth_neighbour", "ball_counts", "prdc", "max_k", "PRDC", "INT_EXACT"]


class PRDC(NamedTuple):
    precision: float
    recall: float
    density: float
    coverage: float
    authenticity: float
    k: int
    n_real: int
    n_synthetic: int
    dim: int
    floor: Optional["PRDC"]


def max_k():
    """The largest ``k`` of ``knn`` (a constant of the library: no device call)."""
    return int(_lib.load().d3p_pair_knn_max_k())


def _check_k(k, what):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= max_k():
        raise ValueError(f"{what}: k must be an int in [1, {max_k()}], got {k!r}")
    return k


def _check_radius(radius_sq, nb, what):
    if not isinstance(radius_sq, torch.Tensor) or radius_sq.dim() != 1 or radius_sq.dtype != torch.float32 or int(radius_sq.shape[0]) != nb:
        raise ValueError(f"{what}: radius_sq: a 1-D float32 CUDA tensor of {nb} squared radii, one per row of b, is required")


def _walk(a, da, b, db, k, exclude, radius_sq):
    """One call of d3p_pair_knn on checked tables."""
    (na, d, a_ld), (nb, _, b_ld) = da, db
    lib = _lib.load()
    dev = a.device
    sq = torch.empty((na, k), dtype=torch.float32, device=dev)
    dist = torch.empty((na, k), dtype=torch.float32, device=dev)
    index = torch.empty((na, k), dtype=torch.int32, device=dev)
    count = torch.empty(na, dtype=torch.int32, device=dev) if radius_sq is not None else None
    rad = radius_sq.contiguous() if radius_sq is not None else None
    need = int(lib.d3p_pair_knn_workspace(na, nb, d, k))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    check(lib.d3p_pair_knn(stream_ptr(), ptr(a), ptr(b), T.dtype_code(a), a_ld, b_ld, na, nb, d, k, 1 if exclude else 0,
                           ptr(rad), ptr(sq), ptr(dist), ptr(index), ptr(count), ptr(ws), int(ws.numel()) if need else 0))
    idx = index.to(torch.int64) & 0xFFFFFFFF
    out = {"distance": dist, "sq": sq, "index": torch.where(idx == 0xFFFFFFFF, torch.full_like(idx, -1), idx)}
    if count is not None:
        c = count.to(torch.int64) & 0xFFFFFFFF
        out["count"] = torch.where(c == 0xFFFFFFFF, torch.full_like(c, -1), c)
    return out


def knn(a, b, k, exclude_diagonal=False, radius_sq=None):
    """Per row of ``a`` its ``k`` nearest rows of ``b`` -- ``{"distance", "sq", "index"}``, each ``(n_a, k)``, ascending -- and with
    ``radius_sq`` (squared radii, one per row of ``b``) ``"count"``: the number of rows of ``b`` whose ball contains it (module
    docstring).  ``exclude_diagonal=True`` leaves out ``j == i`` (a table against itself: ``n_a == n_b``)."""
    what = "knn"
    da, db = T.check_pair(a, b, ("a", "b"), what)
    k = _check_k(k, what)
    exclude = T.check_diagonal(exclude_diagonal, da, db, what)
    if radius_sq is not None:
        _check_radius(radius_sq, db[0], what)
    tables = (("a", a), ("b", b))
    with T.on_device(tables + (("radius_sq", radius_sq),), what, exact=tables):
        return _walk(a, da, b, db, k, exclude, radius_sq)


def kth_neighbour(x, k):
    """The distance of every row of ``x`` to its ``k``-th nearest OTHER row of ``x``: ``{"distance": (n,), "sq": (n,)}`` float32, the
    radius of the row's k-NN ball (``+inf`` where the table has no more than ``k`` rows)."""
    what = "kth_neighbour"
    dx, _ = T.check_pair(x, x, ("x", "x"), what)
    k = _check_k(k, what)
    with T.on_device((("x", x),), what, exact=(("x", x),)):
        out = _walk(x, dx, x, dx, k, True, None)
        return {"distance": out["distance"][:, k - 1], "sq": out["sq"][:, k - 1]}


def ball_counts(a, b, radius_sq):
    """Per row of ``a`` the number of rows ``j`` of ``b`` with ``sq(i, j) < radius_sq[j]``: ``(n_a,)`` int64 (-1: a flagged row)."""
    what = "ball_counts"
    da, db = T.check_pair(a, b, ("a", "b"), what)
    _check_radius(radius_sq, db[0], what)
    tables = (("a", a), ("b", b))
    with T.on_device(tables + (("radius_sq", radius_sq),), what, exact=tables):
        return _walk(a, da, b, db, 1, False, radius_sq)["count"]


def _share(flags):
    """The share of set flags: an integer count over the number of rows, one correctly rounded division."""
    return int(flags.sum()) / flags.numel()


def _prdc(real, dr, synth, ds, k, floor):
    """PRDC from the four walks on checked tables."""
    rr, ss = _walk(real, dr, real, dr, k, True, None), _walk(synth, ds, synth, ds, k, True, None)
    r_real, r_synth = rr["sq"][:, k - 1], ss["sq"][:, k - 1]
    sr, rs = _walk(synth, ds, real, dr, 1, False, r_real), _walk(real, dr, synth, ds, 1, False, r_synth)
    if bool((sr["count"] < 0).any()) or bool((rs["count"] < 0).any()):   # flagged rows: a count of -1 is no count
        raise ValueError("prdc: a table holds a NaN or infinite element: the scores are not defined (knn flags the rows)")
    nearest = sr["index"][:, 0]
    return PRDC(precision=_share(sr["count"] > 0), recall=_share(rs["count"] > 0),
                density=int(sr["count"].sum()) / (k * ds[0]), coverage=_share(rs["sq"][:, 0] < r_real),
                authenticity=_share(sr["sq"][:, 0] > rr["sq"][nearest, 0]), k=k, n_real=dr[0], n_synthetic=ds[0], dim=dr[1], floor=floor)


def prdc(real, synthetic, k=5, holdout=None):
    """Precision, recall, density, coverage and authenticity of ``synthetic`` against ``real`` from k-NN balls (module docstring): a
    ``PRDC``, whose ``floor`` is ``prdc(real, holdout, k)`` when a holdout is given.  These are functions of the PRIVATE tables and are
    not covered by the accountant."""
    what = "prdc"
    tables = T.check_group(real, synthetic, holdout, ("real", "synthetic", "holdout"), what)
    dr, ds, dh = ([dims for _, _, dims in tables] + [None])[:3]
    k = _check_k(k, what)
    for name, _, dims in tables:
        if dims[0] < k + 1:
            raise ValueError(f"{what}: {name}: {dims[0]} rows; at least k + 1 = {k + 1} are required (every row needs k other rows)")
    with T.on_device(tables, what, exact=tables):
        floor = _prdc(real, dr, holdout, dh, k, None) if holdout is not None else None
        return _prdc(real, dr, synthetic, ds, k, floor)
