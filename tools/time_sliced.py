#!/usr/bin/env python3
"""Times the sliced Wasserstein distance's kernels (d3p_project_rows, d3p_column_w2_distance, d3p_amd.sliced) with device events after
three warm-ups (developer tool).

    python tools/time_sliced.py [--reps 21] [--side-limit 20] [--rows 1000000] [--pair-rows 30000]

On resident float32 tables of d = 64 columns (outputs and workspace allocated inside the timed call, as the module does), ALTERNATING in
one process:
  * project(x, theta, shift) onto 128 directions against torch.matmul on the centred table (x - shift) @ theta, at --rows rows;
  * w2_distance of two sorted (128, rows) tables of unequal length against a torch composition (both quantile functions gathered on the
    pooled grid of levels, a float64 sum);
  * sliced_wasserstein(real, synthetic, n_dirs=128) against fidelity.energy_distance at --pair-rows rows, a size both can run.
Before them the tool measures the copy bandwidth (d3p_hbm_copy over 1 GiB) and prints THE FLOOR of the projection derived from it: the
table read once and the projections written once, 4 n (d + L) bytes.  Every side runs under its own time limit (tools/time_fidelity.py).
Per line: microseconds (median, minimum and maximum over the repetitions) and the ratios of the medians.  The figures are recorded, not
gated.  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import fidelity as FD  # noqa: E402
from d3p_amd import sliced as SL  # noqa: E402
from d3p_amd import univariate as UV  # noqa: E402
from tools.time_covariance import copy_bandwidth  # noqa: E402
from tools.time_fidelity import _time_sides  # noqa: E402
from tools.time_waic import _line  # noqa: E402

D, DIRS = 64, 128


def _torch_w2(sa, sb):
    """The squared 2-Wasserstein distance per row of two sorted (d, n) tables: the quantile functions on the pooled levels."""
    n_a, n_b = sa.shape[1], sb.shape[1]
    edges = torch.cat([torch.arange(1, n_a + 1, device=sa.device) * n_b, torch.arange(1, n_b + 1, device=sa.device) * n_a]).unique()
    width = torch.diff(edges, prepend=edges.new_zeros(1)).double()
    start = edges - torch.diff(edges, prepend=edges.new_zeros(1))
    delta = sa[:, start // n_b].double() - sb[:, start // n_a].double()
    return (delta * delta * width).sum(dim=1) / (float(n_a) * float(n_b))


def run(reps, limit_s, rows, pair_rows, bw):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((rows, D), device="cuda", generator=g) + 1000.0
    theta = SL.random_directions(D, DIRS, device="cuda")
    shift = x.double().mean(dim=0).float()
    dx, dt = (rows, D, D), (DIRS, DIRS)
    shape = f"d={D} {rows} rows onto {DIRS} directions, float32"
    floor = round(4.0 * rows * (D + DIRS) / bw * 1e6, 1)
    (t_p, n_p), (t_mm, _) = _time_sides([lambda: SL._project(x, dx, theta, dt, shift), lambda: torch.matmul(x - shift, theta)], reps, limit_s)
    diff = float((SL._project(x, dx, theta, dt, shift) - torch.matmul(x - shift, theta)).abs().max())
    _line(f"d3p_project_rows, {shape}", t_p, {"reps": n_p, "matmul_over_this": round(t_mm[0] / t_p[0], 2), "floor_us_bytes_at_copy_rate": floor,
                                              "this_over_floor": round(t_p[0] / floor, 2), "max_abs_diff_vs_matmul": diff})
    _line(f"torch.matmul(x - shift, theta), {shape}", t_mm, {})
    n_b = rows // 3 + 1
    sa = UV._sort(SL._project(x, dx, theta, dt, shift), (rows, DIRS, DIRS), False)[0]
    sb = UV._sort(SL._project(x[:n_b] * 1.1, (n_b, D, D), theta, dt, shift), (n_b, DIRS, DIRS), False)[0]
    del x
    da, db = (DIRS, rows, rows), (DIRS, n_b, n_b)
    (t_w, n_w), (t_tw, _) = _time_sides([lambda: SL._w2(sa, da, sb, db), lambda: _torch_w2(sa, sb)], reps, limit_s)
    rel = float(((SL._w2(sa, da, sb, db) - _torch_w2(sa, sb)).abs() / _torch_w2(sa, sb)).max())
    shape = f"{DIRS} columns, {rows} against {n_b} sorted values"
    _line(f"d3p_column_w2_distance, {shape}", t_w, {"reps": n_w, "torch_over_this": round(t_tw[0] / t_w[0], 2), "max_rel_diff_vs_torch": rel})
    _line(f"torch composition of W2, {shape}", t_tw, {})
    del sa, sb
    torch.cuda.empty_cache()
    a, b = torch.randn((pair_rows, D), device="cuda", generator=g), torch.randn((pair_rows, D), device="cuda", generator=g) * 1.1
    (t_s, n_s), (t_e, _) = _time_sides([lambda: SL.sliced_wasserstein(a, b, n_dirs=DIRS), lambda: FD.energy_distance(a, b)], reps, limit_s)
    shape = f"d={D} {pair_rows} x {pair_rows} rows"
    _line(f"sliced_wasserstein, {DIRS} directions, {shape}", t_s, {"reps": n_s, "energy_distance_over_this": round(t_e[0] / t_s[0], 2)})
    _line(f"fidelity.energy_distance, {shape}", t_e, {})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--side-limit", type=float, default=20.0, help="seconds of measured time after which a side takes no further turn")
    ap.add_argument("--rows", type=int, default=10 ** 6)
    ap.add_argument("--pair-rows", type=int, default=30000)
    a = ap.parse_args()
    L.require_device()
    bw = copy_bandwidth()
    _line("d3p_hbm_copy, 1 GiB", (0.0, 0.0, 0.0), {"bytes_per_s_read_plus_write": round(bw)})
    run(a.reps, a.side_limit, a.rows, a.pair_rows, bw)


if __name__ == "__main__":
    main()
