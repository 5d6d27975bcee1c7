"""What the table diagnostics share on the host: ``fidelity``, ``permutation``, ``neighbours``, ``marginals``,
``covariance``, ``univariate``, ``mixed``, ``sliced``, ``mmd`` and ``sinkhorn`` take tables ``(rows, d)`` under one ABI, and every
check of such a table, the device entry and the ABI's dtype code have their one definition here.  (A call's workspace stays a
``torch.empty`` of the calling module: the guarded-memory tests hand it out through that module's ``torch``.)

A public function makes its checks in one order: the argument checks (``check_*``, which read shapes, dtypes and strides and never a
value), then ``on_device``, which asks the device question and makes the ONE check that reads the tables.  Every message starts with
``what``, the public function's name.  The module is private: it imports torch, so ``d3p_amd/__init__.py`` does not import it.
"""
import contextlib
import math

import torch

from . import _lib

INT_EXACT = 2 ** 24   # |v| <= 2^24: every int32 the float32 conversion keeps exactly

MAX_ROWS = 2 ** 32 - 2          # of a pair walk (the nearest row's index is a uint32 and 0xFFFFFFFF stands for "none")
MAX_ROWS_SORTED = 2 ** 31 - 1   # of a column sort and of a Gram walk
MAX_ROWS_RANKS = 2 ** 30 - 1    # of the doubled midranks, which are int32
_MEDIAN_ROWS = 1024


# ---------------------------------------------------------------------------------------------------------------- argument checks
def check_row_stride(t, name, what):
    """The row stride of a 1-D or 2-D tensor whose rows may be strided: at least a row's width (a single row: the width)."""
    width = int(t.shape[1]) if t.dim() == 2 else 1
    ld = int(t.stride(0)) if int(t.shape[0]) > 1 else width
    if ld < width:
        raise ValueError(f"{what}: {name}: the rows of the tensor overlap (strides {tuple(t.stride())})")
    return ld


def check_table(t, name, what):
    """(n, d, ld) of one table after the host checks."""
    if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2) or t.dtype not in (torch.float32, torch.int32):
        raise ValueError(f"{what}: {name}: a 2-D float32 or int32 CUDA tensor (rows, d) is required (1-D (rows,): d = 1)")
    n = int(t.shape[0])
    d = int(t.shape[1]) if t.dim() == 2 else 1
    if n < 1:
        raise ValueError(f"{what}: {name}: at least one row")
    if d < 1:
        raise ValueError(f"{what}: {name}: d >= 1 is required")
    if n > MAX_ROWS:
        raise ValueError(f"{what}: {name}: {n} rows; at most {MAX_ROWS} (the nearest row's index is a uint32)")
    if t.dim() == 2 and d > 1 and t.stride(1) != 1:
        raise ValueError(f"{what}: {name}: the columns must have unit stride (the rows may be strided)")
    return n, d, check_row_stride(t, name, what)


def check_match(a, b, d_a, d_b, names, what):
    """Two checked tables of ``d_a`` and ``d_b`` columns have one dtype and one d."""
    if a.dtype != b.dtype:
        raise ValueError(f"{what}: {names[0]} is {a.dtype} and {names[1]} is {b.dtype}: one dtype for both tables")
    if d_a != d_b:
        raise ValueError(f"{what}: {names[0]} has {d_a} columns and {names[1]} has {d_b}: one d for both tables")


def check_pair(a, b, names, what):
    da, db = check_table(a, names[0], what), check_table(b, names[1], what)
    check_match(a, b, da[1], db[1], names, what)
    return da, db


def check_group(real, other, holdout, names, what, against=0):
    """[(name, tensor, (n, d, ld)), ..] of a real table, the table compared with it and, if given, a holdout: ``names`` names the
    three, and the holdout is checked as a pair with table ``against`` of the group (0: the real one, 1: the other)."""
    dr, do = check_pair(real, other, names[:2], what)
    group = [(names[0], real, dr), (names[1], other, do)]
    if holdout is not None:
        dh, _ = check_pair(holdout, group[against][1], (names[2], names[against]), what)
        group.append((names[2], holdout, dh))
    return group


def check_rows(dx, name, what, ranks):
    if dx[0] > MAX_ROWS_SORTED:
        raise ValueError(f"{what}: {name}: {dx[0]} rows; at most 2^31 - 1 are sorted")
    if ranks and dx[0] > MAX_ROWS_RANKS:
        raise ValueError(f"{what}: {name}: {dx[0]} rows; the doubled midranks are int32: at most 2^30 - 1 rows")
    return dx


def check_diagonal(exclude_diagonal, da, db, what):
    if not isinstance(exclude_diagonal, (bool, int)) or exclude_diagonal not in (0, 1):
        raise ValueError(f"{what}: exclude_diagonal must be a bool")
    if exclude_diagonal and da[0] != db[0]:
        raise ValueError(f"{what}: exclude_diagonal compares a table with itself: {da[0]} rows against {db[0]}")
    return bool(exclude_diagonal)


def check_positive(v, name, what):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v > 0 and math.isfinite(v)):
        raise ValueError(f"{what}: {name} must be a finite number > 0, got {v!r}")
    return float(v)


def check_int(v, name, what, low):
    if isinstance(v, bool) or not isinstance(v, int) or v < low:
        raise ValueError(f"{what}: {name} must be an int >= {low}, got {v!r}")
    return v


def check_column_vector(v, name, d, what):
    if v is not None and (not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != (d,) or not v.is_contiguous()):
        raise ValueError(f"{what}: {name} must be None or a contiguous float32 tensor of shape ({d},)")
    return v


# ---------------------------------------------------------------------------------------------------------------- the device entry
def check_devices(tables, what):
    for name, t in tables:
        if not t.is_cuda:
            raise ValueError(f"{what}: {name}: a 2-D float32 or int32 CUDA tensor (rows, d) is required (1-D (rows,): d = 1)")
    if len({t.device for _, t in tables}) != 1:
        raise ValueError(f"{what}: the tables lie on different devices")


def check_exact(tables, what, advice="pass"):
    """The one check that has to read the tables (on the device).  ``energy`` names no tensor (a name of None) and advises to score."""
    for name, t in tables:
        if t.dtype == torch.int32 and bool(((t > INT_EXACT) | (t < -INT_EXACT)).any()):
            raise ValueError(f"{what}: {name + ': ' if name else ''}int32 values beyond 2^24 in magnitude: the kernel converts to float32, "
                             f"which is exact only up to there ({advice} a float32 tensor instead)")


def _named(tables):
    return [(e[0], e[1]) for e in tables if e[1] is not None]


@contextlib.contextmanager
def on_device(tables, what, exact=()):
    """The device entry of a public function, after its argument checks: every tensor of ``tables`` lies on one CUDA device, a device
    is there (``_lib.require_device``: nothing before it needs one), the block runs with that device current, and it starts with the
    exactness check of the tables of ``exact`` -- a subset, possibly empty.  Both are sequences of ``(name, tensor, ..)``; an entry
    whose tensor is None (an optional argument that was not given) is passed over."""
    tables = _named(tables)
    check_devices(tables, what)
    _lib.require_device()   # (every check above runs without a device)
    with torch.cuda.device(tables[0][1].device):
        check_exact(_named(exact), what)
        yield


# ---------------------------------------------------------------------------------------------------------------- the kernel call
def dtype_code(t):
    """The ABI's dtype code of a tensor, or of a torch.dtype: 0 float32, 1 int32."""
    return 0 if getattr(t, "dtype", t) == torch.float32 else 1


# ---------------------------------------------------------------------------------------------------------------- shared summaries
def worst_pairs(diff, top):
    """Of a (d, d) matrix of absolute differences: (the strict upper triangle without its NaNs, the number of NaNs left out, the ``top``
    largest as (((c, e), value), ..))."""
    d = int(diff.shape[0])
    iu = torch.triu_indices(d, d, offset=1, device=diff.device)
    vals = diff[iu[0], iu[1]]
    ok = ~torch.isnan(vals)
    kept = vals[ok]
    worst = ()
    if top and kept.numel():
        w = torch.topk(kept, min(top, kept.numel()))
        at = ok.nonzero().flatten()[w.indices]
        worst = tuple(((int(iu[0][a]), int(iu[1][a])), float(v)) for a, v in zip(at.tolist(), w.values.tolist()))
    return kept, int((~ok).sum()), worst


def median_q(x, y, shift, scale):
    """The median squared distance, in the shifted and scaled space, over the pairs of the pooled strided subsamples (float64)."""
    rows = []
    for t in (x, y):
        n = int(t.shape[0])
        z = t.reshape(n, -1)[::-(-n // _MEDIAN_ROWS)].to(torch.float32) - shift
        rows.append((z * scale if scale is not None else z).to(torch.float64))
    z = torch.cat(rows)
    q = torch.cdist(z, z, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    i, j = torch.triu_indices(z.shape[0], z.shape[0], offset=1, device=z.device)
    return float(q[i, j].median())
