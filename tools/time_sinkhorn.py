#!/usr/bin/env python3
"""Times the soft-min rows (d3p_softmin_rows, d3p_amd.sinkhorn) with device events after three warm-ups (developer tool).

    python tools/time_sinkhorn.py [--reps 21] [--side-limit 20] [--rows 8192] [--dims 2,64,784] [--iters 20]

On resident float32 tables of --rows x --rows rows (outputs and workspace allocated inside the timed call, as the module does),
ALTERNATING in one process, per d of --dims:
  * one softmin_rows walk against one kernel_sums walk at B = 1 on the same tables (the same staging and products: the difference is the
    online epilogue) and against a torch composition that can hold the matrix at this size: torch.cdist (its Gram form) squared and a
    logsumexp -- with the largest difference of the outputs in bits;
  * sinkhorn_divergence(x, y, epsilon, n_iter=--iters, anneal=False) end to end (4 (iters + 1) walks, the moments) against
    fidelity.energy_distance(x, y) (three walks) and mmd.mmd(x, y) (four walks).
Every side runs under its own time limit (tools/time_fidelity.py).  Per line: microseconds (median, minimum and maximum over the
repetitions) and the ratios of the medians.  The figures are recorded, not gated.  Fails without a GPU."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import fidelity as FD  # noqa: E402
from d3p_amd import mmd as M  # noqa: E402
from d3p_amd import sinkhorn as S  # noqa: E402
from tools.time_fidelity import _time_sides  # noqa: E402
from tools.time_waic import _line  # noqa: E402


def _torch_softmin(a, b, gamma, h, shift):
    q = torch.cdist(a - shift, b - shift) ** 2
    return -torch.logsumexp((h[None, :] - gamma * q).double() * math.log(2.0), dim=1) / math.log(2.0)


def run(reps, limit_s, rows, d, iters):
    g = torch.Generator(device="cuda").manual_seed(d)
    a = torch.randn((rows, d), device="cuda", generator=g) + 100.0
    b = torch.randn((rows, d), device="cuda", generator=g) * 1.1 + 100.0
    h = torch.randn(rows, device="cuda", generator=g)
    shift = a.double().mean(dim=0).float()
    dx, gamma = (rows, d, d), 1.0 / (2.0 * math.log(2.0) * 0.05 * 2.0 * d)
    shape = f"d={d} {rows} x {rows} float32"
    (ts, ns), (tk, nk), (tt, nt) = _time_sides([lambda: S._walk(a, dx, b, dx, gamma, h, shift, None, None, 1.0, None),
                                                lambda: M._sums(a, dx, b, dx, gamma, 1, shift, None, False),
                                                lambda: _torch_softmin(a, b, gamma, h, shift)], reps, limit_s)
    got, ref = S._walk(a, dx, b, dx, gamma, h, shift, None, None, 1.0, None)[0], _torch_softmin(a, b, gamma, h, shift)
    _line(f"d3p_softmin_rows, {shape}", ts, {"reps": ns, "pair_columns_per_s": round(rows * rows * d / (ts[0] * 1e-6)),
                                             "this_over_kernel_sums_b1": round(ts[0] / tk[0], 2), "torch_over_this": round(tt[0] / ts[0], 2),
                                             "max_diff_vs_torch_bits": float((got - ref).abs().max())})
    _line(f"d3p_kernel_sums, B = 1, {shape}", tk, {"reps": nk})
    _line(f"torch cdist^2 + logsumexp, {shape}", tt, {"reps": nt})
    del got, ref
    torch.cuda.empty_cache()
    eps = 0.05 * 2.0 * d
    (td, nd), (te, ne), (tm, nm) = _time_sides([lambda: S.sinkhorn_divergence(a, b, epsilon=eps, n_iter=iters, check_every=iters, anneal=False),
                                                lambda: FD.energy_distance(a, b), lambda: M.mmd(a, b)], reps, limit_s)
    _line(f"sinkhorn_divergence, {iters} iterations + 1, four walks each, {shape}", td,
          {"reps": nd, "this_over_energy_distance": round(td[0] / te[0], 2), "this_over_mmd": round(td[0] / tm[0], 2),
           "us_per_walk": round(td[0] / (4.0 * (iters + 1)), 1)})
    _line(f"fidelity.energy_distance, three walks, {shape}", te, {"reps": ne})
    _line(f"mmd, B = 5, four walks, {shape}", tm, {"reps": nm})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--side-limit", type=float, default=20.0, help="seconds of measured time after which a side takes no further turn")
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--dims", default="2,64,784")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    L.require_device()
    for d in (int(s) for s in a.dims.split(",")):
        run(a.reps, a.side_limit, a.rows, d, a.iters)


if __name__ == "__main__":
    main()
