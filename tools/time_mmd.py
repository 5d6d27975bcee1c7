#!/usr/bin/env python3
"""Times the Gaussian-kernel row sums (d3p_kernel_sums, d3p_amd.mmd) with device events after three warm-ups (developer tool).

    python tools/time_mmd.py [--reps 21] [--side-limit 20] [--rows 8192] [--dims 2,64,784]

On resident float32 tables of --rows x --rows rows (outputs and workspace allocated inside the timed call, as the module does),
ALTERNATING in one process, per d of --dims:
  * kernel_sums(a, b, gamma0, 5, shift) against a torch composition that can hold the matrix at this size: torch.cdist (its Gram form)
    squared, exp2 of five multiples, float64 row sums -- with the largest relative difference of the outputs;
  * kernel_sums at B = 1 against B = 5: what the ladder costs;
  * mmd(x, y) (four walks, the moments and the median subsample) against fidelity.energy_distance(x, y) (three walks): both do O(n^2 d)
    work, which makes the energy distance the yardstick.
Every side runs under its own time limit (tools/time_fidelity.py).  Per line: microseconds (median, minimum and maximum over the
repetitions), the ratios of the medians and the pair-columns per second.  The figures are recorded, not gated.  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import fidelity as FD  # noqa: E402
from d3p_amd import mmd as M  # noqa: E402
from tools.time_fidelity import _time_sides  # noqa: E402
from tools.time_waic import _line  # noqa: E402

B = 5


def _torch_sums(a, b, gamma0, shift):
    q = torch.cdist(a - shift, b - shift) ** 2
    return torch.stack([torch.exp2(-gamma0 * 2.0 ** r * q).double().sum(dim=1) for r in range(B)])


def run(reps, limit_s, rows, d):
    g = torch.Generator(device="cuda").manual_seed(d)
    a = torch.randn((rows, d), device="cuda", generator=g) + 100.0
    b = torch.randn((rows, d), device="cuda", generator=g) * 1.1 + 100.0
    shift = a.double().mean(dim=0).float()
    dx, gamma0 = (rows, d, d), 1.0 / (8.0 * d)
    shape = f"d={d} {rows} x {rows} float32"
    (t5, n5), (t1, n1), (tt, nt) = _time_sides([lambda: M._sums(a, dx, b, dx, gamma0, B, shift, None, False),
                                                lambda: M._sums(a, dx, b, dx, gamma0, 1, shift, None, False),
                                                lambda: _torch_sums(a, b, gamma0, shift)], reps, limit_s)
    got, ref = M._sums(a, dx, b, dx, gamma0, B, shift, None, False), _torch_sums(a, b, gamma0, shift)
    _line(f"d3p_kernel_sums, B = {B}, {shape}", t5, {"reps": n5, "pair_columns_per_s": round(rows * rows * d / (t5[0] * 1e-6)),
                                                    "torch_over_this": round(tt[0] / t5[0], 2), "b5_over_b1": round(t5[0] / t1[0], 2),
                                                    "max_rel_diff_vs_torch": float(((got - ref).abs() / ref).max())})
    _line(f"d3p_kernel_sums, B = 1, {shape}", t1, {"reps": n1})
    _line(f"torch cdist^2 + exp2 x {B} + float64 row sums, {shape}", tt, {"reps": nt})
    del got, ref
    torch.cuda.empty_cache()
    (tm, nm), (te, ne) = _time_sides([lambda: M.mmd(a, b, n_bandwidths=B), lambda: FD.energy_distance(a, b)], reps, limit_s)
    _line(f"mmd, B = {B}, four walks, {shape}", tm, {"reps": nm, "energy_distance_over_this": round(te[0] / tm[0], 2),
                                                     "energy_walk_over_mmd_walk": round((te[0] / 3.0) / (tm[0] / 4.0), 2)})
    _line(f"fidelity.energy_distance, three walks, {shape}", te, {"reps": ne})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--side-limit", type=float, default=20.0, help="seconds of measured time after which a side takes no further turn")
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--dims", default="2,64,784")
    a = ap.parse_args()
    L.require_device()
    for d in (int(s) for s in a.dims.split(",")):
        run(a.reps, a.side_limit, a.rows, d)


if __name__ == "__main__":
    main()
