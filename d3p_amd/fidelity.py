"""Fidelity of a synthetic table against the real one: the two-sample energy distance, the distance to the closest record and the
nearest-neighbour adversarial accuracy.

    pair_stats(a, b, exclude_diagonal=False)  -> {"sum": (na,) float64, "min": (na,) float32, "argmin": (na,) int64}
    energy_distance(x, y)                     -> EnergyDistance(d2, d2_unbiased, exy, exx, eyy, n_x, n_y, dim)
    closest_record(synthetic, real)           -> {"distance": (n,) float32, "index": (n,) int64}
    fidelity_report(train, synthetic, holdout=None, probs=(0.05, 0.5, 0.95), schema=None) -> FidelityReport

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

With ``schema=`` (a ``d3p_amd.mixed.MixedSchema``: some columns hold category codes, on which a Euclidean distance means nothing) every
walk of the report is Gower's distance of ``d3p_amd.mixed`` (``d3p_pair_stats_mixed``) and every distance is in its units, rounded to
float32 after the division by the total weight; with ``None`` nothing changes, bit for bit.

Every other host check runs before the device is touched; there is no CPU fallback.
"""
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from . import _tables as T
from . import clipping as CL
from ._lib import check, ptr, stream_ptr
from ._tables import INT_EXACT

__all__ = ["pair_stats", "energy_distance", "closest_record", "fidelity_report", "EnergyDistance", "FidelityReport", "INT_EXACT"]


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
    check(lib.d3p_pair_stats(stream_ptr(), ptr(a), ptr(b), T.dtype_code(a), a_ld, b_ld, na, nb, d, 1 if exclude else 0,
                             ptr(s), ptr(m), ptr(am), ptr(ws), int(ws.numel()) if need else 0))
    idx = am.to(torch.int64) & 0xFFFFFFFF
    return {"sum": s, "min": m, "argmin": torch.where(idx == 0xFFFFFFFF, torch.full_like(idx, -1), idx)}


def pair_stats(a, b, exclude_diagonal=False):
    """Per row of ``a`` the float64 sum of its distances to the rows of ``b``, the distance to its nearest row of ``b`` and that row's
    index (module docstring): ``{"sum", "min", "argmin"}`` on the tables' device.  ``exclude_diagonal=True`` leaves out ``j == i`` (a
    table against itself: ``n_a == n_b``)."""
    what = "pair_stats"
    da, db = T.check_pair(a, b, ("a", "b"), what)
    exclude = T.check_diagonal(exclude_diagonal, da, db, what)
    tables = (("a", a), ("b", b))
    with T.on_device(tables, what, exact=tables):
        return _walk(a, da, b, db, exclude)


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
    dx, dy = T.check_pair(x, y, ("x", "y"), what)
    tables = (("x", x), ("y", y))
    with T.on_device(tables, what, exact=tables):
        xy, xx, yy = _walk(x, dx, y, dy, False), _walk(x, dx, x, dx, True), _walk(y, dy, y, dy, True)
        return _energy(xy["sum"], xx["sum"], yy["sum"], dx[0], dy[0], dx[1])


def closest_record(synthetic, real):
    """The distance to the closest record: per row of ``synthetic`` the distance to its nearest row of ``real`` and that row's index,
    ``{"distance": (n,) float32, "index": (n,) int64}``."""
    what = "closest_record"
    ds, dr = T.check_pair(synthetic, real, ("synthetic", "real"), what)
    tables = (("synthetic", synthetic), ("real", real))
    with T.on_device(tables, what, exact=tables):
        out = _walk(synthetic, ds, real, dr, False)
        return {"distance": out["min"], "index": out["argmin"]}


def _share(flags):
    return float(flags.to(torch.float64).mean())


def fidelity_report(train, synthetic, holdout=None, probs=(0.05, 0.5, 0.95), schema=None):
    """Energy distance, distance to the closest record and nearest-neighbour adversarial accuracy of ``synthetic`` against ``train``
    and, if given, ``holdout`` (module docstring): a ``FidelityReport``.  These are functions of the PRIVATE tables and are not covered
    by the accountant.  With a ``schema`` (``d3p_amd.mixed.mixed_schema``: some columns are categorical) every walk is Gower's distance
    of ``d3p_amd.mixed`` and every distance is in its units; with ``None`` the walks are the Euclidean ones, bit for bit."""
    what = "fidelity_report"
    tables = T.check_group(train, synthetic, holdout, ("train", "synthetic", "holdout"), what, against=1)
    dt, ds, dh = ([dims for _, _, dims in tables] + [None])[:3]
    ps = CL._check_probs(probs)
    walk = _walk
    if schema is not None:
        from . import mixed
        mixed._check_schema(schema, dt[1], what)

        def walk(a, da, b, db, exclude):
            out = mixed._walk(a, da, b, db, exclude, schema)
            return {"sum": out["sum"], "min": out["min"].to(torch.float32), "argmin": out["argmin"]}   # (the profile takes float32)
    with T.on_device(tables, what, exact=tables):
        st, ss, tt = walk(synthetic, ds, train, dt, False), walk(synthetic, ds, synthetic, ds, True), walk(train, dt, train, dt, True)
        ts = walk(train, dt, synthetic, ds, False)
        e_train = _energy(st["sum"], ss["sum"], tt["sum"], ds[0], dt[0], ds[1])
        dcr = st["min"]
        quant = CL.norm_profile(dcr, (), ps).quantiles if ps else ()
        aa_truth, aa_synth = _share(ts["min"] > tt["min"]), _share(dcr > ss["min"])
        aa = 0.5 * (aa_truth + aa_synth)
        e_hold = aa_hold = loss = closer = None
        if holdout is not None:
            sh, hh, hs = walk(synthetic, ds, holdout, dh, False), walk(holdout, dh, holdout, dh, True), walk(holdout, dh, synthetic, ds, False)
            e_hold = _energy(sh["sum"], ss["sum"], hh["sum"], ds[0], dh[0], ds[1])
            aa_hold = 0.5 * (_share(hs["min"] > hh["min"]) + _share(sh["min"] > ss["min"]))
            loss = aa_hold - aa
            closer = float(((dcr < sh["min"]).to(torch.float64) + 0.5 * (dcr == sh["min"]).to(torch.float64)).mean())
        return FidelityReport(e_train, e_hold, ps, tuple(quant), int((dcr == 0).sum()), aa_truth, aa_synth, aa, aa_hold, loss, closer,
                              dt[0], ds[0], dh[0] if dh else None, ds[1])
