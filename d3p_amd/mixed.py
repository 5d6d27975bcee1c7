"""Fidelity of a synthetic table with CATEGORICAL columns: Gower's distance under the pair statistics, the energy distance, the distance
to the closest record and the fidelity report.

    mixed_schema(real, categorical, weights=None)       -> MixedSchema
    pair_stats(a, b, schema, exclude_diagonal=False)    -> {"sum": (na,) float64, "min": (na,) float64, "argmin": (na,) int64}
    energy_distance(x, y, schema)                       -> fidelity.EnergyDistance
    closest_record(synthetic, real, schema)             -> {"distance": (n,) float64, "index": (n,) int64}
    fidelity.fidelity_report(train, synthetic, holdout=None, probs=..., schema=schema)

PRIVACY.  Every number here is computed from the PRIVATE table, without noise -- the schema included: its ranges are the maxima and
minima of the real table's numeric columns.  Releasing a report or a schema, or choosing a model by looking at one, is NOT covered by
the accountant (``DPSVI.get_epsilon``): the accountant covers the noised steps of training and nothing else.  The functions are a
diagnostic for the person who holds the data.

The Euclidean distance of ``d3p_amd.fidelity`` means nothing on a category code: region 7 is not nearer to region 8 than to region 1.
Gower's distance of two rows is

    G(a, b) = ( sum over numeric c of w_c |a_c - b_c| / range_c  +  sum over categorical c of w_c [a_c != b_c] ) / W,    W = sum_c w_c

an L1 plus a Hamming sum.  Both are of negative type, so Szekely & Rizzo's energy distance stays a valid two-sample statistic under
it.  ``mixed_schema`` takes the ranges ``max - min`` from the REAL table in float64 (a constant column gets the scale 0) and the
weights (default 1 each; the categorical columns share ONE weight); ``categorical`` lists the columns that hold codes, integers in
``[0, 255]`` stored in the tables' dtype.  The walk is ``d3p_pair_stats_mixed`` (``d3p_amd/csrc/d3p_pair_mixed.hip``): each table is
packed once -- the numeric columns scaled to float32 words, the codes four to a word -- and the 32 x 32 pair tile of ``d3p_pair_stats``
walks the packed tables in the same order, so its determinism and its special cases hold: a row without an admissible ``j`` gets ``0,
+inf, -1``; a NaN or infinite numeric element, or a categorical element that is not an integer in ``[0, 255]``, in row ``i`` of ``a``
makes that row ``NaN, NaN, -1``, and one anywhere in ``b`` every row.  The kernel's float32 distance ``fmaf(w_cat, m, qn)`` and float64
sums are divided by ``W`` in float64 here: the results are in Gower units, in ``[0, 1]`` for rows within the real table's ranges.

The tables are 2-D CUDA tensors of ONE dtype, float32 or int32, as in ``d3p_amd.fidelity``; int32 values beyond ``2^24`` in magnitude
are a ``ValueError``.  Every other host check runs before the device is touched; there is no CPU fallback.
"""
import ctypes as C
import math
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import _lib
from . import _tables as T
from . import fidelity as F
from ._lib import check, ptr, stream_ptr
from ._tables import INT_EXACT

__all__ = ["MixedSchema", "mixed_schema", "pair_stats", "energy_distance", "closest_record", "INT_EXACT"]


class MixedSchema(NamedTuple):
    kind: Tuple[int, ...]        # per column: 0 numeric, 1 categorical
    scale: Tuple[float, ...]     # per column: weight / range as a float32 value (0 for a constant or a categorical column)
    w_cat: float                 # the weight of a categorical mismatch, a float32 value
    total_weight: float          # W
    ranges: Tuple[float, ...]    # per column: max - min of the real table in float64 (NaN for a categorical column)


def _check_schema(schema, d, what):
    if not isinstance(schema, MixedSchema):
        raise ValueError(f"{what}: schema: a MixedSchema (mixed_schema(real, categorical)) is required")
    if len(schema.kind) != d or len(schema.scale) != d:
        raise ValueError(f"{what}: the schema has {len(schema.kind)} columns and the tables {d}")
    if any(k not in (0, 1) for k in schema.kind):
        raise ValueError(f"{what}: schema.kind must hold 0 (numeric) and 1 (categorical)")
    if any(not (math.isfinite(s) and s >= 0.0) for s in schema.scale) or not (math.isfinite(schema.w_cat) and schema.w_cat >= 0.0):
        raise ValueError(f"{what}: schema.scale and schema.w_cat must be finite and >= 0")
    if not (math.isfinite(schema.total_weight) and schema.total_weight > 0.0):
        raise ValueError(f"{what}: schema.total_weight must be finite and > 0")


def mixed_schema(real, categorical, weights=None):
    """The ``MixedSchema`` of the table ``real`` (rows, d): ``categorical`` lists its categorical columns (distinct indices in ``[0,
    d)``, possibly none or all), ``weights`` is ``None`` (1 each) or ``d`` finite weights ``>= 0`` with a positive sum, equal on the
    categorical columns.  The ranges of the numeric columns are ``max - min`` of ``real`` in float64: functions of the PRIVATE table."""
    what = "mixed_schema"
    n, d, _ = T.check_table(real, "real", what)
    try:
        cats = [int(c) for c in categorical]
        ok = all(isinstance(c, (int, np.integer)) and not isinstance(c, bool) for c in categorical)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"{what}: categorical: a sequence of column indices is required")
    if any(c < 0 or c >= d for c in cats):
        raise ValueError(f"{what}: categorical: an index outside [0, {d})")
    if len(set(cats)) != len(cats):
        raise ValueError(f"{what}: categorical: the indices must be distinct")
    if weights is None:
        w = [1.0] * d
    else:
        try:
            w = [float(v) for v in weights]
        except TypeError:
            w = []
        if len(w) != d or any(not (math.isfinite(v) and v >= 0.0) for v in w):
            raise ValueError(f"{what}: weights: {d} finite weights >= 0 are required")
    if len({w[c] for c in cats}) > 1:
        raise ValueError(f"{what}: weights: the categorical columns share one weight")
    total = math.fsum(w)
    if not total > 0.0:
        raise ValueError(f"{what}: weights: the sum of the weights must be > 0")
    w_cat = float(np.float32(w[cats[0]])) if cats else 0.0
    if not math.isfinite(w_cat):
        raise ValueError(f"{what}: weights: the categorical weight overflows float32")
    kind = [1 if c in set(cats) else 0 for c in range(d)]
    table = real if real.dim() == 2 else real[:, None]
    with T.on_device((("real", real),), what):
        t64 = table.to(torch.float64)
        rng = (t64.max(dim=0).values - t64.min(dim=0).values).cpu().tolist()
    scale, ranges = [], []
    for c in range(d):
        if kind[c]:
            scale.append(0.0)
            ranges.append(float("nan"))
            continue
        if not math.isfinite(rng[c]):
            raise ValueError(f"{what}: real: column {c} holds a NaN or an infinite value")
        s = float(np.float32(w[c] / rng[c])) if rng[c] > 0.0 else 0.0      # float64 quotient, rounded once
        if not math.isfinite(s):
            raise ValueError(f"{what}: real: the scale weight / range of column {c} overflows float32")
        scale.append(s)
        ranges.append(rng[c])
    return MixedSchema(tuple(kind), tuple(scale), w_cat, total, tuple(ranges))


def _walk(a, da, b, db, exclude, schema):
    """One call of d3p_pair_stats_mixed on checked tables: the three per-row outputs in Gower units (float64)."""
    (na, d, a_ld), (nb, _, b_ld) = da, db
    lib = _lib.load()
    dev = a.device
    kind = (C.c_uint8 * d)(*schema.kind)
    scale = (C.c_float * d)(*schema.scale)
    dc = sum(schema.kind)
    s = torch.empty(na, dtype=torch.float64, device=dev)
    m = torch.empty(na, dtype=torch.float32, device=dev)
    am = torch.empty(na, dtype=torch.int32, device=dev)
    need = int(lib.d3p_pair_stats_mixed_workspace(na, nb, d - dc, dc))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    check(lib.d3p_pair_stats_mixed(stream_ptr(), ptr(a), ptr(b), T.dtype_code(a), a_ld, b_ld, na, nb, d,
                                   C.cast(kind, C.c_void_p), C.cast(scale, C.c_void_p), schema.w_cat, 1 if exclude else 0,
                                   ptr(s), ptr(m), ptr(am), ptr(ws), need))
    idx = am.to(torch.int64) & 0xFFFFFFFF
    return {"sum": s / schema.total_weight, "min": m.to(torch.float64) / schema.total_weight,
            "argmin": torch.where(idx == 0xFFFFFFFF, torch.full_like(idx, -1), idx)}


def pair_stats(a, b, schema, exclude_diagonal=False):
    """Per row of ``a`` the float64 sum of its Gower distances to the rows of ``b``, the distance to its nearest row of ``b`` and that
    row's index (module docstring): ``{"sum", "min", "argmin"}`` on the tables' device, the kernel's values divided by ``W`` in float64.
    These are functions of the PRIVATE tables and are not covered by the accountant."""
    what = "mixed.pair_stats"
    da, db = T.check_pair(a, b, ("a", "b"), what)
    _check_schema(schema, da[1], what)
    exclude = T.check_diagonal(exclude_diagonal, da, db, what)
    tables = (("a", a), ("b", b))
    with T.on_device(tables, what, exact=tables):
        return _walk(a, da, b, db, exclude, schema)


def energy_distance(x, y, schema):
    """The two-sample energy distance of the tables ``x`` and ``y`` under Gower's distance (module docstring): ``fidelity.EnergyDistance``
    of 0-d float64 tensors, from the three walks of ``fidelity.energy_distance``.  A function of the PRIVATE tables, not covered by the
    accountant."""
    what = "mixed.energy_distance"
    dx, dy = T.check_pair(x, y, ("x", "y"), what)
    _check_schema(schema, dx[1], what)
    tables = (("x", x), ("y", y))
    with T.on_device(tables, what, exact=tables):
        xy, xx, yy = _walk(x, dx, y, dy, False, schema), _walk(x, dx, x, dx, True, schema), _walk(y, dy, y, dy, True, schema)
        return F._energy(xy["sum"], xx["sum"], yy["sum"], dx[0], dy[0], dx[1])


def closest_record(synthetic, real, schema):
    """The Gower distance to the closest record: per row of ``synthetic`` the distance to its nearest row of ``real`` and that row's
    index, ``{"distance": (n,) float64, "index": (n,) int64}``.  A function of the PRIVATE tables, not covered by the accountant."""
    what = "mixed.closest_record"
    ds, dr = T.check_pair(synthetic, real, ("synthetic", "real"), what)
    _check_schema(schema, ds[1], what)
    tables = (("synthetic", synthetic), ("real", real))
    with T.on_device(tables, what, exact=tables):
        out = _walk(synthetic, ds, real, dr, False, schema)
        return {"distance": out["min"], "index": out["argmin"]}
