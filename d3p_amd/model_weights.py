"""Model weights for M candidate models: stacking of predictive distributions, pseudo-BMA and pseudo-BMA+.

    stacking_weights(results, tol=1e-7, max_iter=20000)          -> ModelWeights
    pseudo_bma_weights(results, rng_key=None, n_boot=1000)       -> ModelWeights
    compare_models(results, method="stacking", **kw)             -> ModelComparison
    stacking_from_matrix(e, tol=1e-7, max_iter=20000)            -> (weights, info)      the model-free layer
    bootstrap_from_matrix(rng_key, e, n_boot=1000)               -> (weights, z)

``results`` maps names to ``criteria.WAICResult`` or ``criteria.LOOResult`` (a dict, or a list that is named ``"0", "1", ..``): all of
one kind, all with ``pointwise=True``, all over the same ``n_rows``; anything else is a ``ValueError``, as for ``criteria.compare``.  The
pointwise ``elpd_loo`` resp. ``elpd_waic`` vectors -- float32, one value per row, on the device -- are stacked into the ``M x rows``
matrix ``e`` the two entries of ``d3p_amd/csrc/d3p_model_weights.hip`` reduce (include/d3p_hip.h states both rules); ``1 <= M <= 16``.

Stacking (Yao, Vehtari, Simpson & Gelman 2018) maximises ``f(w) = sum_r log sum_m w_m exp(e[m, r])`` over the simplex by the EM fixed
point from ``w = 1 / M``; it stops where the duality gap ``max_m g_m - 1 <= tol``, which bounds ``(f(w*) - f(w)) / rows``: a
certificate, not a heuristic.  ``n_iter`` counts the updates applied, ``converged`` is False where ``max_iter`` updates did not reach
``tol``, ``gap`` and ``stacked_elpd = f(w)`` belong to the returned ``weights``.  The iteration runs on the device; the entry reads one
flag per chunk of evaluations, and ``n_iter`` / ``converged`` are read once at the end.

``pseudo_bma_weights`` with ``rng_key=None`` is plain pseudo-BMA: the softmax of the models' total elpd (float64 torch on the device, no
kernel).  With a threefry key it is pseudo-BMA+: ``n_boot`` Bayesian-bootstrap replicates of the totals (``d3p_bb_pseudo_bma``; ``1 <=
n_boot <= 65535``), ``weights`` the mean of the replicates' softmax and ``se_boot`` the standard deviation over the replicates of each
model's bootstrapped elpd (the population form, as ArviZ's).  The ``n_boot x rows`` weights are never written.

Special values: a ``-inf`` in some models of a row is legitimate; a NaN or ``+inf`` anywhere, or a row that is ``-inf`` in every model,
makes every weight NaN.  Nothing is dropped.

``compare_models`` is ArviZ's ``compare`` table on the log scale, sorted by elpd descending: ``rank``, ``elpd``, ``p`` (``p_loo`` /
``p_waic``), ``elpd_diff`` and ``dse`` paired against the best model (``criteria._total_and_se`` of the pointwise differences: the
values of ``criteria.compare(best, other)``), ``weight``, ``se``, and ``warning`` (a ``LOOResult`` with ``n_high_k > 0``).  ``method``
is ``"stacking"``, ``"pseudo-BMA"`` or ``"pseudo-BMA+"`` (the last needs ``rng_key=``).  Mixing the models' predictive DRAWS by the
weights is out of scope here.  Every host check runs before the device is touched; there is no CPU fallback.
"""
from typing import NamedTuple, Optional

import torch

from . import _lib
from . import criteria as CR
from . import modelling as M
from ._lib import check, ptr, stream_ptr

__all__ = ["stacking_weights", "pseudo_bma_weights", "compare_models", "stacking_from_matrix", "bootstrap_from_matrix", "ModelWeights",
           "ModelComparison", "METHODS", "MAX_MODELS", "MAX_BOOT"]

METHODS = ("stacking", "pseudo-BMA", "pseudo-BMA+")
MAX_MODELS = 16
MAX_BOOT = 65535


class ModelWeights(NamedTuple):
    names: tuple
    weights: torch.Tensor                 # (M,) float64 on the device, in the order of names
    method: str                           # one of METHODS
    n_iter: Optional[int]                 # stacking: EM updates applied
    converged: Optional[bool]             # stacking: gap <= tol was reached
    gap: Optional[torch.Tensor]           # stacking: 0-d float64, the duality gap of weights
    stacked_elpd: Optional[torch.Tensor]  # stacking: 0-d float64, f(weights)
    se_boot: Optional[torch.Tensor]       # pseudo-BMA+: (M,) float64, the bootstrap standard error of each model's elpd


class ModelComparison(NamedTuple):
    names: tuple                 # sorted by elpd, best first; every column below is in this order
    rank: tuple                  # 0, 1, ..
    elpd: torch.Tensor           # (M,) float64
    p: torch.Tensor              # (M,) float64: p_loo resp. p_waic
    elpd_diff: torch.Tensor      # (M,) float64: elpd of the best model minus this one's, from the paired pointwise differences
    dse: torch.Tensor            # (M,) float64: its standard error (0 for the best model)
    weight: torch.Tensor         # (M,) float64
    se: torch.Tensor             # (M,) float64: the standard error of elpd
    warning: tuple               # bool per model: a LOOResult with n_high_k > 0
    method: str
    kind: str                    # "loo" or "waic"
    weights: ModelWeights        # in the ORIGINAL order of the results

    def table(self):
        """The comparison as text, one line per model."""
        cols = [c.detach().cpu().tolist() for c in (self.elpd, self.p, self.elpd_diff, self.dse, self.weight, self.se)]
        width = max([5] + [len(n) for n in self.names])
        lines = [f"{'model':<{width}}  rank  {'elpd_' + self.kind:>12}  {'p_' + self.kind:>9}  {'elpd_diff':>10}  {'dse':>8}  {'weight':>7}  "
                 f"{'se':>8}  warning"]
        for i, name in enumerate(self.names):
            e, p, d, ds, w, s = (c[i] for c in cols)
            lines.append(f"{name:<{width}}  {self.rank[i]:>4}  {e:>12.2f}  {p:>9.2f}  {d:>10.2f}  {ds:>8.2f}  {w:>7.3f}  {s:>8.2f}  "
                         f"{self.warning[i]}")
        return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ host checks
def _named(results, what):
    if isinstance(results, dict):
        items = [(str(k), v) for k, v in results.items()]
    elif isinstance(results, (list, tuple)) and not isinstance(results, (CR.WAICResult, CR.LOOResult)):   # (a result is a tuple itself)
        items = [(str(i), v) for i, v in enumerate(results)]
    else:
        raise ValueError(f"{what}: results must be a dict or a list of WAICResult / LOOResult")
    if not 1 <= len(items) <= MAX_MODELS:
        raise ValueError(f"{what}: 1 <= M <= {MAX_MODELS} models are weighted, got {len(items)}")
    first = items[0][1]
    for name, r in items:
        if not isinstance(r, (CR.WAICResult, CR.LOOResult)) or r.pointwise is None:
            raise ValueError(f"{what}: {name!r} must be a WAICResult or a LOOResult with its pointwise arrays (pointwise=True)")
        if type(r) is not type(first):
            raise ValueError(f"{what}: a {type(first).__name__} and a {type(r).__name__} estimate different quantities; weigh results "
                             "of one kind")
        if r.n_rows != first.n_rows:
            raise ValueError(f"{what}: the results cover {first.n_rows} and {r.n_rows} rows; model weights need the same rows")
    if first.n_rows < 1:
        raise ValueError(f"{what}: the results cover no rows")
    site = "elpd_waic" if isinstance(first, CR.WAICResult) else "elpd_loo"
    return tuple(n for n, _ in items), [r for _, r in items], site


def _check_stacking(tol, max_iter, what):
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not tol > 0:
        raise ValueError(f"{what}: tol must be a number > 0, got {tol!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or not 1 <= max_iter <= 2 ** 32 - 2:
        raise ValueError(f"{what}: max_iter must be an int >= 1, got {max_iter!r}")


def _check_boot(n_boot, what):
    if isinstance(n_boot, bool) or not isinstance(n_boot, int) or not 1 <= n_boot <= MAX_BOOT:
        raise ValueError(f"{what}: n_boot must be an int in 1..{MAX_BOOT}, got {n_boot!r}")


def _check_e(e, what):
    """(M, rows, ld) of the models x rows matrix: a 2-D CUDA float32 tensor, any row stride, unit column stride."""
    if not isinstance(e, torch.Tensor) or e.dim() != 2 or e.dtype != torch.float32:
        raise ValueError(f"{what}: e must be a 2-D float32 tensor (models, rows)")
    m, rows = int(e.shape[0]), int(e.shape[1])
    if not 1 <= m <= MAX_MODELS:
        raise ValueError(f"{what}: 1 <= M <= {MAX_MODELS} models are weighted, got {m}")
    if rows < 1:
        raise ValueError(f"{what}: rows >= 1 is required")
    if not e.is_cuda:
        raise ValueError(f"{what}: e must be a CUDA tensor (there is no CPU fallback)")
    if rows > 1 and e.stride(1) != 1:
        raise ValueError(f"{what}: e must have unit column stride")
    ld = int(e.stride(0)) if m > 1 else rows
    if ld < rows:
        raise ValueError(f"{what}: the row stride of e must be >= rows")
    return m, rows, ld


def _matrix(results, site):
    return torch.stack([r.pointwise[site].detach().to(torch.float32).reshape(-1) for r in results])


# ------------------------------------------------------------------------------------------------ the model-free layer
def _stacking(e, m, rows, ld, tol, max_iter):
    lib = _lib.load()
    w = torch.empty((m,), dtype=torch.float64, device=e.device)
    info = torch.empty((4,), dtype=torch.float64, device=e.device)
    nbytes = int(lib.d3p_stacking_workspace(rows, m))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=e.device)
    check(lib.d3p_stacking_weights(stream_ptr(), ptr(e), ld, rows, m, float(tol), int(max_iter), ptr(w), ptr(info), ptr(ws), nbytes))
    return w, info


def _bootstrap(key, e, m, rows, ld, n_boot):
    lib = _lib.load()
    w = torch.empty((m,), dtype=torch.float64, device=e.device)
    z = torch.empty((n_boot, m), dtype=torch.float64, device=e.device)
    nbytes = int(lib.d3p_bb_pseudo_bma_workspace(rows, m, n_boot))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=e.device)
    check(lib.d3p_bb_pseudo_bma(stream_ptr(), ptr(key), ptr(e), ld, rows, m, n_boot, ptr(w), ptr(z), ptr(ws), nbytes))
    return w, z


def stacking_from_matrix(e, tol=1e-7, max_iter=20000):
    """Stacking weights of the rows of ``e`` (models x rows, float32, CUDA): ``(weights, info)``, ``(M,)`` and ``(4,)`` float64 on the
    device, ``info = {n_iter, converged, gap, f}``."""
    what = "stacking_from_matrix"
    _check_stacking(tol, max_iter, what)
    m, rows, ld = _check_e(e, what)
    _lib.require_device()
    with torch.cuda.device(e.device):
        return _stacking(e, m, rows, ld, tol, max_iter)


def bootstrap_from_matrix(rng_key, e, n_boot=1000):
    """Pseudo-BMA+ weights of the rows of ``e`` over ``n_boot`` Bayesian-bootstrap replicates: ``(weights, z)``, ``(M,)`` and ``(n_boot,
    M)`` float64 on the device; ``z[b, m]`` is replicate ``b``'s elpd of model ``m``."""
    what = "bootstrap_from_matrix"
    _check_boot(n_boot, what)
    m, rows, ld = _check_e(e, what)
    key = M._check_key(rng_key)
    _lib.require_device()
    with torch.cuda.device(e.device):
        return _bootstrap(key.to(e.device), e, m, rows, ld, n_boot)


# ------------------------------------------------------------------------------------------------ the results layer
def stacking_weights(results, tol=1e-7, max_iter=20000):
    """Stacking weights of the models in ``results`` (module docstring)."""
    what = "stacking_weights"
    names, rs, site = _named(results, what)
    _check_stacking(tol, max_iter, what)
    _lib.require_device()
    e = _matrix(rs, site)
    m, rows, ld = _check_e(e, what)
    with torch.cuda.device(e.device):
        w, info = _stacking(e, m, rows, ld, tol, max_iter)
        host = info[:2].cpu()      # the one read: n_iter and converged
    return ModelWeights(names, w, "stacking", int(host[0]), bool(host[1] != 0), info[2], info[3], None)


def pseudo_bma_weights(results, rng_key=None, n_boot=1000):
    """Pseudo-BMA weights (``rng_key=None``: the softmax of the total elpd, no kernel) or pseudo-BMA+ weights (a threefry key: the
    Bayesian bootstrap over ``n_boot`` replicates) of the models in ``results`` (module docstring)."""
    what = "pseudo_bma_weights"
    names, rs, site = _named(results, what)
    if rng_key is None:
        _lib.require_device()
        total = _matrix(rs, site).to(torch.float64).sum(dim=1)
        return ModelWeights(names, torch.softmax(total, dim=0), "pseudo-BMA", None, None, None, None, None)
    _check_boot(n_boot, what)
    key = M._check_key(rng_key)
    _lib.require_device()
    e = _matrix(rs, site)
    m, rows, ld = _check_e(e, what)
    with torch.cuda.device(e.device):
        w, z = _bootstrap(key.to(e.device), e, m, rows, ld, n_boot)
        dev = z - z.sum(dim=0) / n_boot
        se = torch.sqrt((dev * dev).sum(dim=0) / n_boot)
    return ModelWeights(names, w, "pseudo-BMA+", None, None, None, None, se)


def compare_models(results, method="stacking", **kw):
    """The comparison table of the models in ``results`` (module docstring).  ``kw`` goes to ``stacking_weights`` (``tol``, ``max_iter``)
    resp. ``pseudo_bma_weights`` (``rng_key``, ``n_boot``)."""
    what = "compare_models"
    names, rs, site = _named(results, what)
    if method not in METHODS:
        raise ValueError(f"{what}: method must be one of {METHODS}, got {method!r}")
    if method == "pseudo-BMA+" and kw.get("rng_key") is None:
        raise ValueError(f"{what}: pseudo-BMA+ needs rng_key= (a threefry key) for the Bayesian bootstrap")
    if method == "pseudo-BMA" and kw:
        raise ValueError(f"{what}: pseudo-BMA takes no further arguments, got {sorted(kw)}")
    named = dict(zip(names, rs))
    if len(named) != len(names):
        raise ValueError(f"{what}: the models' names must differ")
    mw = stacking_weights(named, **kw) if method == "stacking" else pseudo_bma_weights(named, **kw)
    loo = site == "elpd_loo"
    elpd = torch.stack([r.elpd_loo if loo else r.elpd_waic for r in rs]).to(torch.float64)
    order = sorted(range(len(rs)), key=lambda i, v=elpd.cpu().tolist(): (-v[i] if v[i] == v[i] else float("inf"), i))   # NaN last
    best = rs[order[0]]
    pairs = [CR._total_and_se(best.pointwise[site].to(torch.float64) - rs[i].pointwise[site].to(torch.float64)) for i in order]
    idx = torch.tensor(order, device=elpd.device)
    warning = tuple(bool(rs[i].n_high_k > 0) if loo else False for i in order)
    return ModelComparison(tuple(names[i] for i in order), tuple(range(len(order))), elpd[idx],
                           torch.stack([rs[i].p_loo if loo else rs[i].p_waic for i in order]).to(torch.float64),
                           torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs]), mw.weights[idx],
                           torch.stack([rs[i].se for i in order]).to(torch.float64), warning, method, "loo" if loo else "waic", mw)
