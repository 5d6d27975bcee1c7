"""Entropic optimal transport between a synthetic table and a real one: the debiased Sinkhorn divergence of Feydy et al. (2019) from
log-domain iterations whose one primitive, a row-wise soft-min over the other table, is a Gram walk on the matrix cores with an online
log-sum-exp -- four walks an iteration and never the ``n_a x n_b`` matrix.

    softmin_rows(a, b, gamma, h, shift=None, scale=None, prev=None, omega=1.0, logw=None)   -> (pot, out_h)
    sinkhorn_divergence(x, y, epsilon="median", epsilon_share=0.05, wx=None, wy=None, n_iter=200, tol=1e-4, check_every=10,
                        anneal=True, scaling=0.5, scale="std", debias=True)                   -> SinkhornDivergence

PRIVACY.  Every number here is computed from the PRIVATE table, without noise.  Releasing a divergence or a potential, or choosing a
model by looking at one, is NOT covered by the accountant (``DPSVI.get_epsilon``): the accountant covers the noised steps of training
and nothing else.  The functions are a diagnostic for the person who holds the data.

``softmin_rows`` is the kernel call (``d3p_softmin_rows``, ``d3p_amd/csrc/d3p_sinkhorn.hip``).  ``a`` and ``b`` are tables as
``mmd.kernel_sums`` takes them, ``shift`` and ``scale`` contiguous ``(d,)`` float32 tensors or None, ``gamma`` a finite float ``> 0``
(rounded to float32), ``h`` a contiguous ``(n_b,)`` float32 tensor in base-2 units, ``prev`` a contiguous ``(n_a,)`` float64 tensor or
None, ``omega`` a float in ``(0, 1]``, ``logw`` a contiguous ``(n_a,)`` float32 tensor or None.  With ``t = fl32(fl32(x - shift) *
scale)`` and ``q_ij`` the squared distance from the float32 Gram product, clamped at 0,

    L_i   = log2 sum_j 2^(h_j - gamma q_ij)
    pot_i = -L_i,  or  prev_i + omega ((-L_i) - prev_i)  with prev                     float64, (n_a,)
    out_h = float32(pot + logw)  with logw, else None: the h of the opposite walk

``h_j = -inf`` is a row of zero weight; a NaN or ``+inf`` in ``h`` makes every row NaN, a non-finite element in row ``i`` of ``a`` that
row, one in ``b`` every row.  The Gram form moves the exponent by ``gamma`` times the error of ``q``, an absolute error of ``L`` in
bits: pass a ``shift`` near the column means.  The kernel's header derives the bound.  Repeated calls give equal bits.

``sinkhorn_divergence`` compares ``y`` with ``x`` under the cost ``C = |tx - ty|^2 / 2`` in the space ``t`` of ``mmd.mmd`` (the shift
the float32 column mean of ``x``, the scale ``1 / std`` of ``x`` under ``scale="std"``).  ``epsilon="median"`` is ``epsilon_share``
times the median squared distance of ``mmd``'s pooled subsample; a number is taken as given.  ``gamma = 1 / (2 epsilon ln 2)`` and the
potentials are kept in exponent bits, ``phi = f / (epsilon ln 2)``, in float64.  ``wx`` and ``wy`` default to uniform; given weights
(1-D, non-negative, a positive sum) are normalised in float64 and a zero weight is ``-inf`` in ``logw`` and ``h``.  An iteration is the
symmetric averaged step, ``omega = 1/2``, from potentials of 0:

    phi <- (phi + softmin over y with h = psi + log2 wy) / 2        psi <- (psi + softmin over x with h = phi_old + log2 wx) / 2

and with ``debias`` the self-problems ``p <- (p + softmin over x with h = p + log2 wx) / 2`` of each table: four walks, enqueued without
a host synchronisation.  Every ``check_every`` iterations ``max(|d phi|, |d psi|)`` in bits is reduced on the device and read; at most
``tol``, or after ``n_iter`` iterations, one final step with ``omega = 1`` closes.  With ``anneal`` one iteration runs first at each
``epsilon_k`` of the geometric schedule from the squared diameter bound of the transformed tables (the sum of their squared column
ranges) down to ``epsilon`` by the factor ``scaling^2``, the potentials rescaled by ``epsilon_k / epsilon_(k+1)`` between rungs (torch,
a cold path).  Returned:

    divergence       epsilon ln 2 (sum wx (phi - p_x) + sum wy (psi - p_y)), float64 torch; ot_xy with debias=False
    ot_xy            epsilon ln 2 (sum wx phi + sum wy psi)
    f_x, g_y         the potentials in cost units, (n_x,) and (n_y,) float64
    epsilon, n_iter_run (iterations at the last epsilon, without the rungs and the final step), converged
    marginal_error   max_j |2^(psi_old - psi_new) - 1| of the last averaged step over the rows of y with weight

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

__all__ = ["softmin_rows", "sinkhorn_divergence", "SinkhornDivergence", "INT_EXACT"]

_LN2 = math.log(2.0)


class SinkhornDivergence(NamedTuple):
    divergence: torch.Tensor      # () float64
    ot_xy: torch.Tensor           # () float64
    f_x: torch.Tensor             # (n_x,) float64, cost units
    g_y: torch.Tensor             # (n_y,) float64
    epsilon: float
    n_iter_run: int
    converged: bool
    marginal_error: float
    n_x: int
    n_y: int
    dim: int


def _check_rows_vector(v, name, n, dtype, what, optional=True):
    if v is None and optional:
        return v
    if not isinstance(v, torch.Tensor) or v.dtype != dtype or tuple(v.shape) != (n,) or not v.is_contiguous():
        raise ValueError(f"{what}: {name} must be {'None or ' if optional else ''}a contiguous {str(dtype).replace('torch.', '')} tensor of shape ({n},)")
    return v


def _check_omega(omega, what):
    if isinstance(omega, bool) or not isinstance(omega, (int, float)) or not 0.0 < omega <= 1.0:
        raise ValueError(f"{what}: omega must be a number in (0, 1], got {omega!r}")
    return float(omega)


def _walk(a, da, b, db, gamma, h, shift, scale, prev, omega, logw):
    """One call of d3p_softmin_rows on checked arguments: (pot, out_h)."""
    (na, d, a_ld), (nb, _, b_ld) = da, db
    lib = _lib.load()
    pot = torch.empty(na, dtype=torch.float64, device=a.device)
    out_h = torch.empty(na, dtype=torch.float32, device=a.device) if logw is not None else None
    ws = torch.empty(int(lib.d3p_softmin_rows_workspace(na, nb)), dtype=torch.uint8, device=a.device)
    check(lib.d3p_softmin_rows(stream_ptr(), ptr(a), ptr(b), T.dtype_code(a), a_ld, b_ld, na, nb, d, ptr(shift), ptr(scale),
                               gamma, ptr(h), ptr(prev), omega, ptr(logw), ptr(pot), ptr(out_h), ptr(ws), int(ws.numel())))
    return pot, out_h


def softmin_rows(a, b, gamma, h, shift=None, scale=None, prev=None, omega=1.0, logw=None):
    """Per row of ``a`` the negated base-2 log-sum-exp of ``h_j - gamma q_ij`` over the rows of ``b``, averaged with ``prev`` by
    ``omega``, and with ``logw`` the float32 ``h`` of the opposite walk (module docstring): ``(pot, out_h)`` on the tables' device."""
    what = "softmin_rows"
    da, db = T.check_pair(a, b, ("a", "b"), what)
    T.check_rows(da, "a", what, False)
    T.check_rows(db, "b", what, False)
    gamma = T.check_positive(gamma, "gamma", what)
    _check_rows_vector(h, "h", db[0], torch.float32, what, optional=False)
    T.check_column_vector(shift, "shift", da[1], what)
    T.check_column_vector(scale, "scale", da[1], what)
    _check_rows_vector(prev, "prev", da[0], torch.float64, what)
    omega = _check_omega(omega, what)
    _check_rows_vector(logw, "logw", da[0], torch.float32, what)
    tables = (("a", a), ("b", b))
    with T.on_device(tables + (("h", h), ("shift", shift), ("scale", scale), ("prev", prev), ("logw", logw)), what, exact=tables):
        return _walk(a, da, b, db, gamma, h, shift, scale, prev, omega, logw)


def _check_weights(w, name, n, what):
    if w is not None and (not isinstance(w, torch.Tensor) or not w.dtype.is_floating_point or tuple(w.shape) != (n,)):
        raise ValueError(f"{what}: {name} must be None or a floating-point tensor of shape ({n},)")
    return w


def _log_weights(w, n, device, name, what):
    """(w normalised in float64, log2 w as float32 with -inf at a zero weight)."""
    if w is None:
        w = torch.full((n,), 1.0 / n, dtype=torch.float64, device=device)
    else:
        w = w.to(torch.float64)
        total = float(w.sum())
        if not (bool((w >= 0).all()) and total > 0 and math.isfinite(total)):
            raise ValueError(f"{what}: {name} must be non-negative and finite with a positive sum")
        w = w / total
    return w, torch.log2(w).to(torch.float32)


def _schedule(diameter2, epsilon, scaling):
    """The rungs above ``epsilon``: diameter2 scaling^(2 k) while that is > epsilon."""
    rungs, e = [], float(diameter2)
    while e > epsilon and len(rungs) < 200:
        rungs.append(e)
        e *= scaling * scaling
    return rungs


def sinkhorn_divergence(x, y, epsilon="median", epsilon_share=0.05, wx=None, wy=None, n_iter=200, tol=1e-4, check_every=10, anneal=True,
                        scaling=0.5, scale="std", debias=True):
    """The debiased Sinkhorn divergence of ``y`` against ``x`` under ``C = |tx - ty|^2 / 2`` at regularisation ``epsilon``, with its
    potentials (module docstring): a ``SinkhornDivergence``.  These are functions of the PRIVATE tables and are not covered by the
    accountant."""
    what = "sinkhorn_divergence"
    dx, dy = T.check_pair(x, y, ("x", "y"), what)
    T.check_rows(dx, "x", what, False)
    T.check_rows(dy, "y", what, False)
    if not (isinstance(epsilon, str) and epsilon == "median"):
        if isinstance(epsilon, str):
            raise ValueError(f"{what}: epsilon must be 'median' or a finite number > 0, got {epsilon!r}")
        epsilon = T.check_positive(epsilon, "epsilon", what)
    epsilon_share = T.check_positive(epsilon_share, "epsilon_share", what)
    _check_weights(wx, "wx", dx[0], what)
    _check_weights(wy, "wy", dy[0], what)
    T.check_int(n_iter, "n_iter", what, 1)
    T.check_int(check_every, "check_every", what, 1)
    tol = T.check_positive(tol, "tol", what)
    if isinstance(scaling, bool) or not isinstance(scaling, (int, float)) or not 0.0 < scaling < 1.0:
        raise ValueError(f"{what}: scaling must be a number in (0, 1), got {scaling!r}")
    if not (scale is None or (isinstance(scale, str) and scale == "std")):
        raise ValueError(f"{what}: scale must be 'std' or None, got {scale!r}")
    tables = (("x", x), ("y", y))
    with T.on_device(tables + (("wx", wx), ("wy", wy)), what, exact=tables):
        dev = x.device
        wxn, lwx = _log_weights(wx, dx[0], dev, "wx", what)
        wyn, lwy = _log_weights(wy, dy[0], dev, "wy", what)
        shift, inv_std = CV.standardise(x, dx)
        if scale is not None:
            scale = inv_std.to(torch.float32)
        if isinstance(epsilon, str):
            epsilon = epsilon_share * T.median_q(x, y, shift, scale)
            if not (epsilon > 0 and math.isfinite(epsilon)):
                raise ValueError(f"{what}: the median squared distance of the subsample gives epsilon = {epsilon}: pass an epsilon")
        rungs = []
        if anneal:
            lo, hi = [], []
            for t, dt in ((x, dx), (y, dy)):
                z = t.reshape(dt[0], -1).to(torch.float32) - shift
                z = z * scale if scale is not None else z
                lo.append(z.min(dim=0).values)
                hi.append(z.max(dim=0).values)
            span = (torch.maximum(*hi) - torch.minimum(*lo)).to(torch.float64)
            rungs = _schedule(float((span * span).sum()), epsilon, float(scaling))

        sides = [(x, dx, y, dy, lwx), (y, dy, x, dx, lwy)] + ([(x, dx, x, dx, lwx), (y, dy, y, dy, lwy)] if debias else [])
        # the potentials in bits: phi, psi and, with debias, p_x, p_y; h[k] = float32(pot[k] + log2 w): the h of the walk that reads side k
        pot = [torch.zeros(s[1][0], dtype=torch.float64, device=dev) for s in sides]
        reads = (1, 0, 2, 3)       # walk k reads the h made from potential reads[k]: phi <- psi, psi <- phi_old, p <- p

        def hs():
            return [(p + s[4]).to(torch.float32) for p, s in zip(pot, sides)]

        def step(eps, h, omega, averaged=True):
            g = 1.0 / (2.0 * eps * _LN2)
            out = [_walk(s[0], s[1], s[2], s[3], g, h[reads[k]], shift, scale, pot[k] if averaged else None, omega, s[4]) for k, s in enumerate(sides)]
            return [o[0] for o in out], [o[1] for o in out]

        h = hs()
        for k, eps in enumerate(rungs):
            pot, h = step(eps, h, 0.5)
            nxt = rungs[k + 1] if k + 1 < len(rungs) else epsilon
            pot = [p * (eps / nxt) for p in pot]
            h = hs()
        converged, n_run, last_psi = False, 0, pot[1]
        for it in range(n_iter):
            old = pot
            pot, h = step(epsilon, h, 0.5)
            n_run, last_psi = it + 1, old[1]
            if (it + 1) % check_every == 0:
                delta = torch.maximum(torch.nan_to_num(pot[0] - old[0], posinf=0.0).abs().max(), torch.nan_to_num(pot[1] - old[1], posinf=0.0).abs().max())
                if float(delta) <= tol:
                    converged = True
                    break
        live = wyn > 0
        marginal = float((torch.exp2(last_psi - pot[1]) - 1.0).abs()[live].max())
        pot, _ = step(epsilon, h, 1.0, averaged=False)
        scale_c = epsilon * _LN2
        ot = scale_c * (torch.sum(wxn * pot[0]) + torch.sum(wyn * pot[1]))
        div = scale_c * (torch.sum(wxn * (pot[0] - pot[2])) + torch.sum(wyn * (pot[1] - pot[3]))) if debias else ot
        return SinkhornDivergence(div, ot, pot[0] * scale_c, pot[1] * scale_c, float(epsilon), n_run, converged, marginal, dx[0], dy[0], dx[1])
