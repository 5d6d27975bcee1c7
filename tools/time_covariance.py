#!/usr/bin/env python3
"""Times the column-moments entry (d3p_column_moments, d3p_amd.covariance) with device events after three warm-ups (developer tool).

    python tools/time_covariance.py [--reps 21] [--side-limit 20] [--shapes 0,1,2]

d3p_column_moments alone on a resident table (outputs and workspace allocated inside the timed call, as the module does), at
  0  the mixture example's shape   d = 2,    10^5 rows (float32)
  1  BASELINE config 3's shape     d = 64,   10^6 rows (float32)
  2  VAE-like images               d = 784,  6 x 10^4 rows (int32 in {0, 1})
ALTERNATING in one process with the two references to beat: the float64 composition `xd = x.double(); xd -= xd.mean(0); xd.T @ xd`, and
float32 torch.cov (whose largest relative difference to the float64 composition is reported: the columns carry means of 1000 times
their spread, where a float32 Gram form cancels).

Before the shapes the tool measures the copy bandwidth (d3p_hbm_copy over 1 GiB) and prints THE FLOORS derived from it: two reads of the
table at that bandwidth, and n d^2 / 2 multiply-adds at the matrix instruction's documented rate (v_mfma_f32_32x32x2_f32: 2048
multiply-adds in 64 cycles on each of 4 SIMDs of 256 CUs at 2.4 GHz).  Every side runs under its own time limit: once its measured
repetitions add up to --side-limit seconds it takes no further turn.  Per line: microseconds (median, minimum and maximum over the
repetitions) and the ratios of the medians.  The figures are recorded, not gated.  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import covariance as CV  # noqa: E402
from tools.time_fidelity import _event_us, _time_sides  # noqa: E402
from tools.time_waic import _line  # noqa: E402

SHAPES = (("mixture example", 2, 10 ** 5, torch.float32), ("config 3", 64, 10 ** 6, torch.float32), ("VAE-like", 784, 6 * 10 ** 4, torch.int32))
MFMA_MACS_PER_S = 2048 / 64 * 4 * 256 * 2.4e9      # multiply-adds per second of the float32 matrix instruction on the whole chip
COPY_BYTES = 2 ** 30


def copy_bandwidth(reps=7):
    """Bytes per second of d3p_hbm_copy (read + write counted) over 1 GiB: the median of `reps` after one warm-up."""
    lib = L.load()
    n = COPY_BYTES // 4
    src, dst = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    src.fill_(1.0)
    run = lambda: L.check(lib.d3p_hbm_copy(L.stream_ptr(), L.ptr(dst), L.ptr(src), COPY_BYTES, 16))  # noqa: E731
    run()
    ts = sorted(_event_us(run) for _ in range(reps))
    return 2.0 * COPY_BYTES / (ts[len(ts) // 2] * 1e-6)


def _float64_composition(x):
    xd = x.double()
    xd -= xd.mean(0)
    return xd.T @ xd


def kernel_alone(reps, limit_s, which, bw):
    g = torch.Generator(device="cuda").manual_seed(0)
    for idx in which:
        name, d, n, dtype = SHAPES[idx]
        if dtype == torch.int32:
            x = torch.randint(0, 2, (n, d), device="cuda", generator=g, dtype=torch.int32)
        else:
            x = torch.randn((n, d), device="cuda", generator=g) + 1000.0
        dx = (n, d, d)
        floors = {"floor_us_two_reads": round(2.0 * n * d * 4 / bw * 1e6, 1), "floor_us_matrix_rate": round(n * d * d / 2 / MFMA_MACS_PER_S * 1e6, 1)}
        shape = f"{name}: d={d} {n} rows, {str(dtype).replace('torch.', '')}"
        _line(f"floors, {shape}", (0.0, 0.0, 0.0), floors)
        xf = x.float()
        sides = [lambda: CV._moments(x, dx), lambda: _float64_composition(x), lambda: torch.cov(xf.T)]
        (t_this, n_this), (t_f64, n_f64), (t_cov, n_cov) = _time_sides(sides, reps, limit_s)
        got, ref, f32 = CV._moments(x, dx).m2, _float64_composition(x), torch.cov(xf.T).double() * (n - 1)
        scale = torch.sqrt(torch.diagonal(ref)[:, None] * torch.diagonal(ref)[None, :])
        extra = {"reps": n_this, "float64_over_this": round(t_f64[0] / t_this[0], 2), "torch_cov_over_this": round(t_cov[0] / t_this[0], 2),
                 "max_scaled_m2_diff_vs_float64": float(((got - ref).abs() / scale).max()),
                 "workspace_bytes": int(L.load().d3p_column_moments_workspace(n, d))}
        extra.update(floors)
        _line(f"d3p_column_moments, {shape}", t_this, extra)
        _line(f"x.double() - mean, xd.T @ xd, {shape}", t_f64, {"reps": n_f64})
        _line(f"float32 torch.cov, {shape}", t_cov, {"reps": n_cov, "max_scaled_m2_diff_vs_float64": float(((f32 - ref).abs() / scale).max())})
        del x, xf, got, ref, f32
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--side-limit", type=float, default=20.0, help="seconds of measured time after which a side takes no further turn")
    ap.add_argument("--shapes", default="0,1,2", help="comma-separated indices of the shapes to run")
    a = ap.parse_args()
    L.require_device()
    bw = copy_bandwidth()
    _line("d3p_hbm_copy, 1 GiB", (0.0, 0.0, 0.0), {"bytes_per_s_read_plus_write": round(bw)})
    kernel_alone(a.reps, a.side_limit, [int(s) for s in a.shapes.split(",")], bw)


if __name__ == "__main__":
    main()
