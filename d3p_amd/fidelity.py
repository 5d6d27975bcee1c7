"""Fidelity of a synthetic table against the real one: the two-sample energy distance, the distance to the closest record and the
nearest-neighbour adversarial accuracy.

    pair_stats(a, b, exclude_diagonal=False)  -> {"sum": (na,) float64, "min": (na,) float32, "argmin": (na,) int64}
    energy_distance(x, y)                     -> EnergyDistance(d2, d2_unbiased, exy, exx, eyy, n_x, n_y, dim)
    closest_record(synthetic, real)           -> {"distance": (n,) float32, "index": (n,) int64}
    fidelity_report(train, synthetic, holdout=None, probs=(0.05, 0.5, 0.95)) -> FidelityReport

PRIVACY.  Every number here is computed from the PRIVATE table, without noise.  Releasing a report, or choosing a model by looking at
it, is NOT covered by the accountant (``DPSVI.get_epsilon``): the accountant covers the noised steps of training and nothing else.  The
functions are a diagnostic for the person who holds the data.

A synthetic TABLE is one draw per row -- ``mixture.posterior_predictive_samples(key, 1, ...)["obs"][0]`` --, where ``d3p_amd.energy``
scores many draws of ONE row against that row's observation.  Three questions come before such a table is released, and all three
reduce one ``O(n_a n_b d)`` walk over the pairs of two tables (``d3p_pair_stats``, ``d3p_amd/csrc/d3p_pair_stats.hip``), which keeps
per row of the first table the float64 sum of its distances to the second and its nearest row there, without the ``n_a x n_b`` matrix:

  * does the synthetic table have the real table's distribution?  The energy distance of Szekely & Rizzo, ``D^2 = 2 E|X - Y| -
    E|X - X'| - E|Y - Y'|`` with the Euclidean norm of ``d3p_amd.energy``: zero only for equal distributions;
  * did the model memorise records?  The distance to the closest record (DCR), each synthetic row's nearest real row, and the share of
    synthetic rows that lie closer to the training split than to a held-out split (about 1/2 when nothing is memorised);
  * can a nearest-neighbour adversary tell the tables apart?  The adversarial accuracy of Yale et al. (2020): 0.5 is indistinguishable,
    1 underfit, 0 copied; its train-minus-holdout gap is their privacy loss.

``pair_stats`` is the model-free reduction.  ``a`` and ``b`` are 2-D CUDA tensors ``(n, d)`` of one dtype, float32 or int32, on one
device, with unit column stride and any row stride ``>= d``; a 1-D tensor is ``d = 1``.  With ``dist`` the float32 distance rule of the
kernel's header (``t = fl32(a_c - b_c)``, an fmaf chain over the columns, ``sqrtf``), for row ``i`` over all ``j < n_b`` -- without ``j ==
i`` when ``exclude_diagonal`` is set, which needs ``n_a == n_b``; duplicate rows are pairs like any other --

    sum[i] = sum_j dist(i, j) in float64, in one fixed order      min[i] = the smallest dist      argmin[i] = the smallest such j

(the tie rule is on the squared distance, not the rounded root).  A row without an admissible ``j`` gets ``0, +inf, -1``; a NaN or
infinite element in row ``i`` of ``a`` makes that row ``NaN, NaN, -1`` and one anywhere in ``b`` every row.  The per-row outputs are
deterministic to the bit and depend on that row, ``b`` and the flag alone.  int32 values are converted to float32 on the device, which
is exact up to ``2^24`` in magnitude: larger values are a ``ValueError`` (this one check reads the tables, so it runs on the device,
after every other).  The workspace is allocated with ``torch.empty``.

``energy_distance`` takes its sums from ``pair_stats(x, y)``, ``pair_stats(x, x, True)`` and ``pair_stats(y, y, True)``: ``exy``, ``exx``
and ``eyy`` with the V-statistic denominators ``n_x n_y``, ``n_x^2`` and ``n_y^2``, ``d2 = 2 exy - exx - eyy`` (>= 0 up to rounding, 0
for equal tables), and ``d2_unbiased`` with ``n (n - 1)`` in the within-table means (NaN when a table has one row).  The closing totals
are ``torch.sum`` in float64 and carry no bit promise; only the per-row outputs do.  The whole ``x x x`` walk is done, not the ``i < j``
half: twice the minimal work, which leaves ``min`` and ``argmin`` of the same walk ready for ``fidelity_report``, which recomputes
nothing.

``fidelity_report`` holds, for ``T`` = train, ``S`` = synthetic, ``H`` = holdout and ``d_AB(i)`` the distance of row ``i`` of ``A`` to
its nearest row of ``B`` (``d_AA``: the diagonal excluded):

    energy_train, energy_holdout   EnergyDistance(S, T) and EnergyDistance(S, H) (None without a holdout)
    dcr_probs, dcr_quantiles       ``clipping.norm_profile`` of d_ST at ``probs``: numpy's ``method='linear'`` on exact order statistics
    n_exact_copies                 #{j : d_ST(j) == 0}
    aa_truth, aa_synth, aa         mean 1[d_TS(i) > d_TT(i)],  mean 1[d_ST(j) > d_SS(j)],  their mean
    aa_holdout, privacy_loss       the same with H for T, and aa_holdout - aa (None without a holdout)
    closer_to_train                the share of S with d_ST(j) < d_SH(j), a tie counting 1/2 (None without a holdout)
    n_train, n_synthetic, n_holdout, dim

Every other host check runs before the device is touched; there is no CPU fallback.
"""
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from . import clipping as CL
from ._lib import check, ptr, stream_ptr
from .energy import INT_EXACT

__all__ = ["pair_stats", "energy_distance", "closest_record", "fidelity_report", "EnergyDistance", "FidelityReport", "INT_EXACT"]

_MAX_ROWS = 2 ** 32 - 2   # (argmin is a uint32 and 0xFFFFFFFF stands for "none")


class EnergyDistance(NamedTuple):
    d2: torch.Tensor             # 0-d float64: 2 exy - exx - eyy, V-statistic
    d2_unbiased: torch.Tensor    # with n (n - 1) in exx and eyy (NaN when a table has one row)
    exy: torch.Tensor            # mean distance between a row of x and a row of y
    exx: torch.Tensor            # mean distance between two rows of x, over n_x^2 pairs (the diagonal's zeros included)
    eyy: torch.Tensor
    n_x: int
    n_y: int
    dim: int


class FidelityReport(NamedTuple):
    energy_train: EnergyDistance
    energy_holdout: Optional[EnergyDistance]
    dcr_probs: Tuple[float, ...]
    dcr_quantiles: Tuple[float, ...]
    n_exact_copies: int
    aa_truth: float
    aa_synth: float
    aa: float
    aa_holdout: Optional[float]
    privacy_loss: Optional[float]
    closer_to_train: Optional[float]
    n_train: int
    n_synthetic: int
    n_holdout: Optional[int]
    dim: int


def _check_table(t, name, what):
    """(n, d, ld) of one table after the host checks."""
    if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2) or t.dtype not in (torch.float32, torch.int32):
        raise ValueError(f"{what}: {name}: a 2-D float32 or int32 CUDA tensor (rows, d) is required (1-D (rows,): d = 1)")
    n = int(t.shape[0])
    d = int(t.shape[1]) if t.dim() == 2 else 1
    if n < 1:
        raise ValueError(f"{what}: {name}: at least one row")
    if d < 1:
        raise ValueError(f"{what}: {name}: d >= 1 is required")
    if n > _MAX_ROWS:
        raise ValueError(f"{what}: {name}: {n} rows; at most {_MAX_ROWS} (the nearest row's index is a uint32)")
    if t.dim() == 2 and d > 1 and t.stride(1) != 1:
        raise ValueError(f"{what}: {name}: the columns must have unit stride (the rows may be strided)")
    ld = int(t.stride(0)) if n > 1 else d
    if ld < d:
        raise ValueError(f"{what}: {name}: the rows of the tensor overlap (strides {tuple(t.stride())})")
    return n, d, ld


def _check_pair(a, b, names, what):
    da, db = _check_table(a, names[0], what), _check_table(b, names[1], what)
    if a.dtype != b.dtype:
        raise ValueError(f"{what}: {names[0]} is {a.dtype} and {names[1]} is {b.dtype}: one dtype for both tables")
    if da[1] != db[1]:
        raise ValueError(f"{what}: {names[0]} has {da[1]} columns and {names[1]} has {db[1]}: one d for both tables")
    return da, db


def _check_devices(tables, what):
    for name, t in tables:
        if not t.is_cuda:
            raise ValueError(f"{what}: {name}: a 2-D float32 or int32 CUDA tensor (rows, d) is required (1-D (rows,): d = 1)")
    if len({t.device for _, t in tables}) != 1:
        raise ValueError(f"{what}: the tables lie on different devices")


def _check_exact(tables, what):
    """The one check that has to read the tables (on the device)."""
    for name, t in tables:
        if t.dtype == torch.int32 and bool(((t > INT_EXACT) | (t < -INT_EXACT)).any()):
            raise ValueError(f"{what}: {name}: int32 values beyond 2^24 in magnitude: the kernel converts to float32, which is exact only "
                             "up to there (pass a float32 tensor instead)")


def _walk(a, da, b, db, exclude):
    """One call of d3p_pair_stats on checked tables: the three per-row outputs."""
    (na, d, a_ld), (nb, _, b_ld) = da, db
    lib = _lib.load()
    dev = a.device
    s = torch.empty(na, dtype=torch.float64, device=dev)
    m = torch.empty(na, dtype=torch.float32, device=dev)
    am = torch.empty(na, dtype=torch.int32, device=dev)
    need = int(lib.d3p_pair_stats_workspace(na, nb, d))
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    check(lib.d3p_pair_stats(stream_ptr(), ptr(a), ptr(b), 0 if a.dtype == torch.float32 else 1, a_ld, b_ld, na, nb, d, 1 if exclude else 0,
                             ptr(s), ptr(m), ptr(am), ptr(ws), int(ws.numel()) if need else 0))
    idx = am.to(torch.int64) & 0xFFFFFFFF
    return {"sum": s, "min": m, "argmin": torch.where(idx == 0xFFFFFFFF, torch.full_like(idx, -1), idx)}


def pair_stats(a, b, exclude_diagonal=False):
    """Per row of ``a`` the float64 sum of its distances to the rows of ``b``, the distance to its nearest row of ``b`` and that row's
    index (module docstring): ``{"sum", "min", "argmin"}`` on the tables' device.  ``exclude_diagonal=True`` leaves out ``j == i`` (a
    table against itself: ``n_a == n_b``)."""
    what = "pair_stats"
    da, db = _check_pair(a, b, ("a", "b"), what)
    if not isinstance(exclude_diagonal, (bool, int)) or exclude_diagonal not in (0, 1):
        raise ValueError(f"{what}: exclude_diagonal must be a bool")
    if exclude_diagonal and da[0] != db[0]:
        raise ValueError(f"{what}: exclude_diagonal compares a table with itself: {da[0]} rows against {db[0]}")
    _check_devices((("a", a), ("b", b)), what)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(a.device):
        _check_exact((("a", a), ("b", b)), what)
        return _walk(a, da, b, db, bool(exclude_diagonal))


def _energy(sxy, sxx, syy, nx, ny, d):
    """EnergyDistance from the per-row sums of the three walks."""
    txy, txx, tyy = torch.sum(sxy), torch.sum(sxx), torch.sum(syy)
    exy, exx, eyy = txy / (nx * ny), txx / (nx * nx), tyy / (ny * ny)
    ux = txx / torch.tensor(float(nx * (nx - 1)), dtype=torch.float64, device=txx.device)      # (0 / 0 = NaN at one row)
    uy = tyy / torch.tensor(float(ny * (ny - 1)), dtype=torch.float64, device=tyy.device)
    return EnergyDistance(2.0 * exy - exx - eyy, 2.0 * exy - ux - uy, exy, exx, eyy, nx, ny, d)


def energy_distance(x, y):
    """The two-sample energy distance of the tables ``x`` and ``y`` (module docstring): ``EnergyDistance`` of 0-d float64 tensors.  The
    whole ``x x x`` and ``y x y`` walks are done, not their ``i < j`` halves: twice the minimal work, and what ``fidelity_report`` needs
    of them is then ready."""
    what = "energy_distance"
    dx, dy = _check_pair(x, y, ("x", "y"), what)
    _check_devices((("x", x), ("y", y)), what)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(x.device):
        _check_exact((("x", x), ("y", y)), what)
        xy, xx, yy = _walk(x, dx, y, dy, False), _walk(x, dx, x, dx, True), _walk(y, dy, y, dy, True)
        return _energy(xy["sum"], xx["sum"], yy["sum"], dx[0], dy[0], dx[1])


def closest_record(synthetic, real):
    """The distance to the closest record: per row of ``synthetic`` the distance to its nearest row of ``real`` and that row's index,
    ``{"distance": (n,) float32, "index": (n,) int64}``."""
    what = "closest_record"
    ds, dr = _check_pair(synthetic, real, ("synthetic", "real"), what)
    _check_devices((("synthetic", synthetic), ("real", real)), what)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(synthetic.device):
        _check_exact((("synthetic", synthetic), ("real", real)), what)
        out = _walk(synthetic, ds, real, dr, False)
        return {"distance": out["min"], "index": out["argmin"]}


def _share(flags):
    return float(flags.to(torch.float64).mean())


def fidelity_report(train, synthetic, holdout=None, probs=(0.05, 0.5, 0.95)):
    """Energy distance, distance to the closest record and nearest-neighbour adversarial accuracy of ``synthetic`` against ``train``
    and, if given, ``holdout`` (module docstring): a ``FidelityReport``.  These are functions of the PRIVATE tables and are not covered
    by the accountant."""
    what = "fidelity_report"
    dt, ds = _check_pair(train, synthetic, ("train", "synthetic"), what)
    tables = [("train", train), ("synthetic", synthetic)]
    dh = None
    if holdout is not None:
        dh, _ = _check_pair(holdout, synthetic, ("holdout", "synthetic"), what)
        tables.append(("holdout", holdout))
    ps = CL._check_probs(probs)
    _check_devices(tables, what)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(train.device):
        _check_exact(tables, what)
        st, ss, tt = _walk(synthetic, ds, train, dt, False), _walk(synthetic, ds, synthetic, ds, True), _walk(train, dt, train, dt, True)
        ts = _walk(train, dt, synthetic, ds, False)
        e_train = _energy(st["sum"], ss["sum"], tt["sum"], ds[0], dt[0], ds[1])
        dcr = st["min"]
        quant = CL.norm_profile(dcr, (), ps).quantiles if ps else ()
        aa_truth, aa_synth = _share(ts["min"] > tt["min"]), _share(dcr > ss["min"])
        aa = 0.5 * (aa_truth + aa_synth)
        e_hold = aa_hold = loss = closer = None
        if holdout is not None:
            sh, hh, hs = _walk(synthetic, ds, holdout, dh, False), _walk(holdout, dh, holdout, dh, True), _walk(holdout, dh, synthetic, ds, False)
            e_hold = _energy(sh["sum"], ss["sum"], hh["sum"], ds[0], dh[0], ds[1])
            aa_hold = 0.5 * (_share(hs["min"] > hh["min"]) + _share(sh["min"] > ss["min"]))
            loss = aa_hold - aa
            closer = float(((dcr < sh["min"]).to(torch.float64) + 0.5 * (dcr == sh["min"]).to(torch.float64)).mean())
        return FidelityReport(e_train, e_hold, ps, tuple(quant), int((dcr == 0).sum()), aa_truth, aa_synth, aa, aa_hold, loss, closer,
                              dt[0], ds[0], dh[0] if dh else None, ds[1])
