"""Binned one- and two-way marginal fidelity of a synthetic table: WHICH columns, and which pairs of columns, a model gets wrong
(DESIGN.md section 4x).

    bin_edges(reference, bins=16, kind="quantile")   -> BinEdges(edges, nbins, max_bins)
    marginal_counts(x, edges, max_bytes=2**30)       -> MarginalCounts(one_way (d, K), two_way (P, K, K), pairs (P, 2), n)
    marginal_fidelity(real, synthetic, bins=16, kind="quantile", columns=None, holdout=None, top=5) -> MarginalFidelity

PRIVACY.  Every number here is computed from the PRIVATE table, without noise -- the bin edges included, which are order statistics of
the real table.  Releasing a report, or choosing a model by looking at it, is NOT covered by the accountant (``DPSVI.get_epsilon``): the
accountant covers the noised steps of training and nothing else.  The functions are a diagnostic for the person who holds the data.

``d3p_amd.fidelity`` answers with GLOBAL numbers (energy distance, closest record).  This module cuts every column into at most 32 bins
and counts, per column, the histogram of the bin codes and, per pair of columns ``i < j``, their ``K x K`` contingency table -- the
k-way marginals (k = 1, 2) of the DP synthetic-data literature, the "contingency similarity" of SDMetrics-style reports.  A categorical
column with integer codes is binned like a continuous one (``kind="integer"``), so mixed-type tables need nothing else.  The counts are
ONE call of ``d3p_marginals`` (``d3p_amd/csrc/d3p_marginals.hip``): ``n d (d - 1) / 2`` integer increments into LDS histograms, never a
one-hot matrix and never a launch per pair.

THE RULE (the kernel's header, word for word).  Column ``c`` has ``nbins[c]`` bins, ``1 <= nbins[c] <= max_bins = B <= 32``, cut by
``nbins[c] - 1`` finite, non-decreasing float32 edges ``edges[c, :nbins[c] - 1]``.  The code of a value ``v`` is ``B`` (the MISSING cell)
if ``v`` is NaN, otherwise ``#{k : e_k < v}`` -- ``numpy.searchsorted(e, v, side="left")``: right-closed bins, ``-inf`` in bin 0,
``+inf`` in the last, ``-0.0 == 0.0``.  The cell stride is ``K = B + 1``.  ``one_way[c, u]`` counts the rows with code ``u`` in column
``c``; ``two_way[p, u, v]`` the rows with code ``u`` in column ``pairs[p, 0]`` and ``v`` in ``pairs[p, 1]``, the pairs ``i < j`` in
lexicographic order (``p = i (2 d - i - 1) / 2 + (j - i - 1)``).  The counts are integers (int64 tensors) and carry the module's only
promise: equal arguments give equal counts, whatever the strides or the order of the device's atomic adds.

``bin_edges`` cuts at places taken from the REFERENCE (real) table only, so that both tables are cut alike.  It is ``torch.sort``
plumbing, runs once and carries no performance claim.  ``edges`` and ``nbins`` of a ``BinEdges`` are CPU tensors ``(d, max(B - 1, 1))``
float32 (unused slots 0) and ``(d,)`` int64.
  * ``kind="quantile"``: per column the distinct values among the order statistics at ranks ``ceil(k m / bins) - 1``, ``k = 1 .. bins -
    1``, of the column's ``m`` finite values -- stored values, no interpolation --, without an edge equal to the column's maximum (its bin
    would be empty).  A column with few distinct values gets fewer bins; one without a finite value gets one.
  * ``kind="uniform"``: ``bins - 1`` equal-width edges between the finite minimum and maximum (one bin where they coincide).
  * ``kind="integer"``: one bin per integer ``min .. max`` of a column (the table int32 or integral-valued); a range above ``bins`` is
    refused.
  * ``bins`` may instead be a list of ``d`` edge sequences of the caller's (finite, non-decreasing, at most 31 each); ``kind`` is then
    ignored and ``max_bins`` is the longest sequence's bin count.

``marginal_counts`` validates its table as ``fidelity.pair_stats`` does (a 2-D float32 or int32 CUDA tensor, unit column stride, rows
that do not overlap; int32 beyond ``2^24`` in magnitude refused, last and on the device) and its ``BinEdges`` on the host (finite,
non-decreasing, ``nbins`` in range) before anything is launched, and refuses a ``two_way`` above ``max_bytes`` (``P K^2 4`` bytes; 1 GiB
by default), naming the size.  Workspace (``n d`` bytes of uint8 codes) and outputs are ``torch.empty``; the entry zeroes the outputs.

``marginal_fidelity`` computes, from the counts of ``real`` and ``synthetic`` under the edges of ``real``, in float64 torch (no bit
promise on these floats; only the counts carry one):

    tvd_one_way (d,), tvd_two_way (P,)     1/2 sum |p - q| over the K (K^2) cells, p and q the counts over their table's rows
    tvd_one_way_mean, tvd_two_way_mean     their means (NaN over no pairs: d = 1)
    worst_columns, worst_pairs             the ``top`` largest: ((column, tvd), ..) and (((i, j), tvd), ..), by the caller's column ids
    cramers_v_real, cramers_v_synthetic    (P,) Cramer's V of every pair's table: sqrt(chi^2 / (n (min(r, c) - 1))) with r and c the
                                           numbers of NON-EMPTY rows and columns (the missing cell is a category like any other);
                                           a table with fewer than two non-empty rows or columns is DEFINED as V = 0
    assoc_diff_mean, assoc_diff_max        mean and max of |V_real - V_synthetic| (NaN over no pairs)
    missing_real, missing_synthetic        (d,) the share of rows in the missing cell
    floor                                  with a ``holdout``: the same report for holdout against real (its own ``floor`` None) -- what
                                           a fresh sample of the SAME distribution scores; a TVD is unreadable without it
    pairs, columns, edges, n_real, n_synthetic

``columns`` gathers a subset of the columns into a contiguous copy first.  Identical tables give every TVD ``== 0`` exactly.  Every
host check runs before the device is touched; there is no CPU fallback.
"""
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .fidelity import INT_EXACT, _check_devices, _check_exact, _check_table

__all__ = ["bin_edges", "marginal_counts", "marginal_fidelity", "BinEdges", "MarginalCounts", "MarginalFidelity", "MAX_BINS", "INT_EXACT"]

MAX_BINS = 32            # d3p_marginals_max_bins()
_KINDS = ("quantile", "uniform", "integer")
_CHUNK_CELLS = 1 << 22   # cells of the pair tables the float64 summaries hold at once


class BinEdges(NamedTuple):
    edges: torch.Tensor      # (d, max(max_bins - 1, 1)) float32, CPU: row c holds nbins[c] - 1 edges, then zeros
    nbins: torch.Tensor      # (d,) int64, CPU
    max_bins: int            # B: the cell stride is B + 1


class MarginalCounts(NamedTuple):
    one_way: torch.Tensor    # (d, K) int64
    two_way: torch.Tensor    # (P, K, K) int64
    pairs: torch.Tensor      # (P, 2) int64: i < j in lexicographic order
    n: int


class MarginalFidelity(NamedTuple):
    tvd_one_way: torch.Tensor
    tvd_two_way: torch.Tensor
    tvd_one_way_mean: float
    tvd_two_way_mean: float
    worst_columns: Tuple[Tuple[int, float], ...]
    worst_pairs: Tuple[Tuple[Tuple[int, int], float], ...]
    cramers_v_real: torch.Tensor
    cramers_v_synthetic: torch.Tensor
    assoc_diff_mean: float
    assoc_diff_max: float
    missing_real: torch.Tensor
    missing_synthetic: torch.Tensor
    floor: Optional["MarginalFidelity"]
    pairs: torch.Tensor
    columns: Tuple[int, ...]
    edges: BinEdges
    n_real: int
    n_synthetic: int


# ---------------------------------------------------------------------------------------------------------------- host checks
def _check_bins(bins, what):
    if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= MAX_BINS:
        raise ValueError(f"{what}: bins must be an int in [1, {MAX_BINS}] or a list of per-column edge sequences, got {bins!r}")
    return bins


def _check_kind(kind, what):
    if kind not in _KINDS:
        raise ValueError(f"{what}: kind must be one of {_KINDS}, got {kind!r}")
    return kind


def _pack(rows, what):
    """BinEdges from per-column lists of float edges, checked: finite, non-decreasing, at most MAX_BINS - 1 each."""
    import math
    B = 1
    for c, e in enumerate(rows):
        if len(e) > MAX_BINS - 1:
            raise ValueError(f"{what}: column {c}: {len(e)} edges; at most {MAX_BINS - 1} ({MAX_BINS} bins)")
        for k, v in enumerate(e):
            if not math.isfinite(v):
                raise ValueError(f"{what}: column {c}: edge {k} is {v}: the edges must be finite")
            if k and v < e[k - 1]:
                raise ValueError(f"{what}: column {c}: the edges decrease at {k} ({e[k - 1]} > {v}): non-decreasing edges are required")
        B = max(B, len(e) + 1)
    edges = torch.zeros((len(rows), max(B - 1, 1)), dtype=torch.float32)
    for c, e in enumerate(rows):
        if len(e):
            edges[c, :len(e)] = torch.tensor(e, dtype=torch.float32)
    for c, e in enumerate(rows):     # (the float32 rounding is monotone, so the order survives it; an overflow to inf does not pass)
        if len(e) and not bool(torch.isfinite(edges[c, :len(e)]).all()):
            raise ValueError(f"{what}: column {c}: an edge is not finite in float32")
    return edges, torch.tensor([len(e) + 1 for e in rows], dtype=torch.int64), B


def _given_edges(seqs, d, what):
    if not isinstance(seqs, (list, tuple)) or len(seqs) != d:
        raise ValueError(f"{what}: a list of {d} per-column edge sequences is required (one per column)")
    rows = []
    for c, e in enumerate(seqs):
        try:
            rows.append([float(v) for v in (e.tolist() if hasattr(e, "tolist") else e)])
        except (TypeError, ValueError):
            raise ValueError(f"{what}: column {c}: a sequence of numbers is required") from None
    edges, nbins, B = _pack(rows, what)
    return BinEdges(edges, nbins, B)


def _check_edges(be, d, what):
    """A BinEdges as the kernel will see it, checked on the host: (edges (d, B - 1 or 1) float32 CPU, nbins (d,) int64 CPU, B)."""
    if not isinstance(be, BinEdges):
        raise ValueError(f"{what}: edges: a BinEdges (bin_edges(reference, ...)) is required")
    e, nb, B = be
    if isinstance(B, bool) or not isinstance(B, int) or not 1 <= B <= MAX_BINS:
        raise ValueError(f"{what}: edges: max_bins must be an int in [1, {MAX_BINS}], got {B!r}")
    if not isinstance(e, torch.Tensor) or not isinstance(nb, torch.Tensor) or e.is_cuda or nb.is_cuda or e.dtype != torch.float32 or \
            nb.dtype != torch.int64 or e.dim() != 2 or nb.dim() != 1 or e.shape[1] != max(B - 1, 1):
        raise ValueError(f"{what}: edges: CPU tensors edges (d, {max(B - 1, 1)}) float32 and nbins (d,) int64 are required")
    if e.shape[0] != d or nb.shape[0] != d:
        raise ValueError(f"{what}: edges: made for {int(e.shape[0])} columns, the table has {d}")
    if bool(((nb < 1) | (nb > B)).any()):
        raise ValueError(f"{what}: edges: nbins must lie in [1, {B}]")
    used = torch.arange(e.shape[1])[None, :] < (nb - 1)[:, None]
    if not bool(torch.isfinite(e[used]).all()):
        raise ValueError(f"{what}: edges: the edges must be finite")
    if e.shape[1] > 1 and bool(((e[:, 1:] < e[:, :-1]) & used[:, 1:]).any()):
        raise ValueError(f"{what}: edges: non-decreasing edges are required")
    return e.contiguous(), nb.contiguous(), B


def _check_columns(columns, d, what):
    if columns is None:
        return None
    try:
        cols = [c for c in columns]
    except TypeError:
        raise ValueError(f"{what}: columns must be a sequence of distinct column indices") from None
    if not cols or any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < d for c in cols) or len(set(cols)) != len(cols):
        raise ValueError(f"{what}: columns must be a non-empty sequence of distinct column indices in [0, {d})")
    return cols


def _two_way_bytes(d, B):
    return d * (d - 1) // 2 * (B + 1) * (B + 1) * 4


def _check_size(d, B, max_bytes, what):
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, int) or max_bytes < 0:
        raise ValueError(f"{what}: max_bytes must be a non-negative int")
    need = _two_way_bytes(d, B)
    if need > max_bytes:
        raise ValueError(f"{what}: the {d * (d - 1) // 2} pair tables of {B + 1} x {B + 1} cells take {need} bytes, above max_bytes = "
                         f"{max_bytes}: fewer bins, a subset of the columns, or a larger max_bytes")


def _as2d(t):
    return t if t.dim() == 2 else t[:, None]


# ---------------------------------------------------------------------------------------------------------------- bin edges
def _edges_on_device(x, bins, kind, what):
    """The per-column edge lists of ``kind`` from the checked CUDA table x (n, d)."""
    v = _as2d(x).to(torch.float64)
    fin = torch.isfinite(v)
    m = fin.sum(dim=0)                                                     # finite values per column
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=v.device)
    lo = torch.where(fin, v, inf).amin(dim=0).cpu().tolist()
    hi = torch.where(fin, v, -inf).amax(dim=0).cpu().tolist()
    mh = m.cpu().tolist()
    d = v.shape[1]
    if kind == "integer":
        if bool((fin & (v != torch.floor(v))).any()):
            raise ValueError(f"{what}: kind='integer' needs an int32 or integral-valued table")
        rows = []
        for c in range(d):
            if mh[c] == 0:
                rows.append([])
                continue
            if hi[c] - lo[c] + 1 > bins:
                raise ValueError(f"{what}: column {c}: the integers {int(lo[c])} .. {int(hi[c])} need {int(hi[c] - lo[c]) + 1} bins, above "
                                 f"bins = {bins}")
            rows.append([lo[c] + k for k in range(int(hi[c] - lo[c]))])
        return rows
    if kind == "uniform":
        return [[] if mh[c] == 0 or not hi[c] > lo[c] else [lo[c] + (hi[c] - lo[c]) * k / bins for k in range(1, bins)] for c in range(d)]
    srt = torch.sort(torch.where(fin, v, inf), dim=0).values              # the m finite values first, ascending
    k = torch.arange(1, bins, device=v.device, dtype=torch.int64)[:, None]
    rank = ((k * m[None, :] + bins - 1) // bins - 1).clamp_(min=0)        # ceil(k m / bins) - 1
    cand = torch.gather(srt, 0, rank).t().cpu().tolist() if bins > 1 else [[] for _ in range(d)]
    return [[] if mh[c] == 0 else sorted({e for e in cand[c] if e < hi[c]}) for c in range(d)]


def bin_edges(reference, bins=16, kind="quantile"):
    """The places at which ``reference`` (the REAL table) cuts its columns (module docstring): ``BinEdges(edges, nbins, max_bins)`` of CPU
    tensors.  ``bins``: the number of bins per column, or a list of per-column edge sequences (then ``kind`` is ignored and the table is
    not read)."""
    what = "bin_edges"
    _, d, _ = _check_table(reference, "reference", what)
    if isinstance(bins, (list, tuple)):
        return _given_edges(bins, d, what)
    bins, kind = _check_bins(bins, what), _check_kind(kind, what)
    _check_devices((("reference", reference),), what)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(reference.device):
        _check_exact((("reference", reference),), what)
        rows = _edges_on_device(reference, bins, kind, what)
    edges, nbins, _ = _pack(rows, what)
    full = torch.zeros((d, max(bins - 1, 1)), dtype=torch.float32)
    full[:, :edges.shape[1]] = edges[:, :full.shape[1]]
    return BinEdges(full, nbins, bins)


# ---------------------------------------------------------------------------------------------------------------- the kernel call
def _counts(x, dims, e, nb, B):
    """One call of d3p_marginals on a checked table with checked edges."""
    n, d, ld = dims
    lib = _lib.load()
    dev = x.device
    K, P = B + 1, d * (d - 1) // 2
    e_dev = e.to(dev)
    nb_dev = nb.to(torch.int32).to(dev)
    one = torch.empty((d, K), dtype=torch.int32, device=dev)
    two = torch.empty((max(P, 1), K, K), dtype=torch.int32, device=dev)
    need = int(lib.d3p_marginals_workspace(n, d, B))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    check(lib.d3p_marginals(stream_ptr(), ptr(x), 0 if x.dtype == torch.float32 else 1, ld, n, d, B, ptr(nb_dev), ptr(e_dev), ptr(one), ptr(two),
                            ptr(ws), int(ws.numel())))
    one, two = one.to(torch.int64), two[:P].to(torch.int64)
    if n >= 2 ** 31:     # (the outputs are uint32)
        one, two = one & 0xFFFFFFFF, two & 0xFFFFFFFF
    iu = torch.triu_indices(d, d, 1, device=dev)
    return MarginalCounts(one, two, iu.t().contiguous(), n)


def marginal_counts(x, edges, max_bytes=2 ** 30):
    """The one-way and two-way counts of the table ``x`` cut at ``edges`` (module docstring): ``MarginalCounts`` of int64 tensors on the
    table's device.  This is the kernel call."""
    what = "marginal_counts"
    dims = _check_table(x, "x", what)
    e, nb, B = _check_edges(edges, dims[1], what)
    _check_size(dims[1], B, max_bytes, what)
    _check_devices((("x", x),), what)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(x.device):
        _check_exact((("x", x),), what)
        return _counts(x, dims, e, nb, B)


# ---------------------------------------------------------------------------------------------------------------- the summaries
def _tvd(ca, na, cb, nb_):
    """1/2 sum |p - q| over the last dimension of two count matrices, in float64."""
    return 0.5 * (ca.to(torch.float64) / na - cb.to(torch.float64) / nb_).abs().sum(dim=-1)


def _cramers_v(tab, n):
    """Cramer's V of (p, K, K) count tables over n rows each; 0 where fewer than two rows or columns are non-empty."""
    o = tab.to(torch.float64)
    r, c = o.sum(dim=2), o.sum(dim=1)
    ex = r[:, :, None] * c[:, None, :] / n
    pos = ex > 0
    chi2 = torch.where(pos, (o - ex) ** 2 / torch.where(pos, ex, torch.ones_like(ex)), torch.zeros_like(ex)).sum(dim=(1, 2))
    k = torch.minimum((r > 0).sum(dim=1), (c > 0).sum(dim=1)) - 1
    v = torch.sqrt(chi2 / (n * k.clamp(min=1).to(torch.float64)))
    return torch.where(k > 0, v, torch.zeros_like(v)).clamp_(max=1.0)


def _mean(t):
    return float(t.mean()) if t.numel() else float("nan")


def _report(cr, cs, B, top, columns, edges):
    """MarginalFidelity (floor None) from the counts of the real and of the other table."""
    K = B + 1
    P = cr.two_way.shape[0]
    tvd1 = _tvd(cr.one_way, cr.n, cs.one_way, cs.n)
    tvd2 = torch.empty(P, dtype=torch.float64, device=tvd1.device)
    vr, vs = torch.empty_like(tvd2), torch.empty_like(tvd2)
    step = max(1, _CHUNK_CELLS // (K * K))
    for lo in range(0, P, step):
        a, b = cr.two_way[lo:lo + step], cs.two_way[lo:lo + step]
        tvd2[lo:lo + step] = _tvd(a.reshape(a.shape[0], K * K), cr.n, b.reshape(b.shape[0], K * K), cs.n)
        vr[lo:lo + step], vs[lo:lo + step] = _cramers_v(a, cr.n), _cramers_v(b, cs.n)
    diff = (vr - vs).abs()
    pairs = cr.pairs
    w1 = torch.topk(tvd1, min(top, tvd1.numel())) if top else None
    w2 = torch.topk(tvd2, min(top, P)) if top and P else None
    ph = pairs.cpu().tolist()
    worst_c = tuple((columns[i], v) for i, v in zip(w1.indices.tolist(), w1.values.tolist())) if w1 is not None else ()
    worst_p = tuple(((columns[ph[i][0]], columns[ph[i][1]]), v) for i, v in zip(w2.indices.tolist(), w2.values.tolist())) if w2 is not None else ()
    return MarginalFidelity(tvd1, tvd2, _mean(tvd1), _mean(tvd2), worst_c, worst_p, vr, vs, _mean(diff), float(diff.max()) if P else float("nan"),
                            cr.one_way[:, B].to(torch.float64) / cr.n, cs.one_way[:, B].to(torch.float64) / cs.n, None, pairs, tuple(columns),
                            edges, cr.n, cs.n)


def marginal_fidelity(real, synthetic, bins=16, kind="quantile", columns=None, holdout=None, top=5, max_bytes=2 ** 30):
    """The binned one- and two-way marginal fidelity of ``synthetic`` against ``real`` -- and, with a ``holdout``, the noise floor that
    holdout against real scores -- cut at the edges of ``real`` (module docstring): a ``MarginalFidelity``.  These are functions of the
    PRIVATE tables and are not covered by the accountant."""
    what = "marginal_fidelity"
    tables = [("real", real), ("synthetic", synthetic)] + ([("holdout", holdout)] if holdout is not None else [])
    dims = [_check_table(t, name, what) for name, t in tables]
    for (name, t), dm in zip(tables[1:], dims[1:]):
        if t.dtype != real.dtype:
            raise ValueError(f"{what}: real is {real.dtype} and {name} is {t.dtype}: one dtype for all tables")
        if dm[1] != dims[0][1]:
            raise ValueError(f"{what}: real has {dims[0][1]} columns and {name} has {dm[1]}: one d for all tables")
    cols = _check_columns(columns, dims[0][1], what)
    d = len(cols) if cols is not None else dims[0][1]
    given = None
    if isinstance(bins, (list, tuple)):
        given = _given_edges(bins, d, what)
    else:
        _check_bins(bins, what)
        _check_kind(kind, what)
    if isinstance(top, bool) or not isinstance(top, int) or top < 0:
        raise ValueError(f"{what}: top must be a non-negative int")
    _check_size(d, given.max_bins if given else bins, max_bytes, what)
    _check_devices(tables, what)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(real.device):
        _check_exact(tables, what)
        if cols is not None:     # a contiguous copy of the chosen columns
            idx = torch.tensor(cols, dtype=torch.int64, device=real.device)
            tables = [(name, _as2d(t).index_select(1, idx).contiguous()) for name, t in tables]
            dims = [(dm[0], d, d) for dm in dims]
        edges = given if given is not None else bin_edges(tables[0][1], bins, kind)
        e, nb, B = _check_edges(edges, d, what)
        counts = [_counts(t, dm, e, nb, B) for (_, t), dm in zip(tables, dims)]
        ids = cols if cols is not None else list(range(d))
        rep = _report(counts[0], counts[1], B, top, ids, edges)
        if holdout is not None:
            rep = rep._replace(floor=_report(counts[0], counts[2], B, top, ids, edges))
        return rep
