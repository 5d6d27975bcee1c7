#!/usr/bin/env python3
"""Times the column sort and the distances on it (d3p_sort_columns, d3p_column_cdf_distance, d3p_amd.univariate) with device events after
three warm-ups (developer tool).

    python tools/time_univariate.py [--reps 21] [--side-limit 20] [--shapes 0,1,2]

On a resident table (outputs and workspace allocated inside the timed call, as the module does), at
  0  the mixture example's shape   d = 2,    10^5 rows (float32)
  1  BASELINE config 3's shape     d = 64,   10^6 rows (float32)
  2  VAE-like counts               d = 784,  6 x 10^4 rows (int32)
ALTERNATING in one process: the sort alone against torch.sort(x, dim=0); the sort with the doubled midranks against torch.sort plus
two searchsorted; cdf_distance of two such tables against a torch composition (sort both, two searchsorted on the pooled values, a
float64 sum).

Before the shapes the tool measures the copy bandwidth (d3p_hbm_copy over 1 GiB) and prints THE FLOOR derived from it: the sort moves
(1 + 3 * 4 + 1) * 4 n d bytes (the key write, per pass a count read, a scatter read and a scatter write, and pass 0's count read, which
is not fused into the key write).  Every side runs under its own time limit (tools/time_fidelity.py).  Per line: microseconds (median,
minimum and maximum over the repetitions) and the ratios of the medians.  The figures are recorded, not gated.  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import univariate as UV  # noqa: E402
from tools.time_covariance import copy_bandwidth  # noqa: E402
from tools.time_fidelity import _time_sides  # noqa: E402
from tools.time_waic import _line  # noqa: E402

SHAPES = (("mixture example", 2, 10 ** 5, torch.float32), ("config 3", 64, 10 ** 6, torch.float32), ("VAE-like", 784, 6 * 10 ** 4, torch.int32))


def _torch_ranks(x):
    s = torch.sort(x, dim=0).values.T.contiguous()
    xt = x.T.contiguous()
    return torch.searchsorted(s, xt, right=False) + torch.searchsorted(s, xt, right=True) + 1


def _torch_cdf(a, b):
    sa, sb = torch.sort(a, dim=0).values.T.contiguous(), torch.sort(b, dim=0).values.T.contiguous()
    pooled = torch.sort(torch.cat([sa, sb], dim=1), dim=1).values
    fa = torch.searchsorted(sa, pooled, right=True).double() / sa.shape[1]
    fb = torch.searchsorted(sb, pooled, right=True).double() / sb.shape[1]
    gap = (fa - fb).abs()
    return gap.max(dim=1).values, (gap[:, :-1] * torch.diff(pooled.double(), dim=1)).sum(dim=1)


def run(reps, limit_s, which, bw):
    g = torch.Generator(device="cuda").manual_seed(0)
    for idx in which:
        name, d, n, dtype = SHAPES[idx]
        if dtype == torch.int32:
            x, y = (torch.randint(0, 40, (n, d), device="cuda", generator=g, dtype=torch.int32) for _ in range(2))
        else:
            x, y = (torch.randn((n, d), device="cuda", generator=g) for _ in range(2))
        dx = (n, d, d)
        shape = f"{name}: d={d} {n} rows, {str(dtype).replace('torch.', '')}"
        floor = round(14.0 * 4 * n * d / bw * 1e6, 1)
        _line(f"floor, {shape}", (0.0, 0.0, 0.0), {"floor_us_sort_bytes_at_copy_rate": floor})
        sides = [lambda: UV._sort(x, dx, False), lambda: torch.sort(x, dim=0), lambda: UV._sort(x, dx, True), lambda: _torch_ranks(x),
                 lambda: UV._cdf(UV._sort(x, dx, False)[0], UV._sort(y, dx, False)[0]), lambda: _torch_cdf(x, y)]
        (t_s, n_s), (t_ts, _), (t_r, _), (t_tr, _), (t_c, _), (t_tc, _) = _time_sides(sides, reps, limit_s)
        assert torch.equal(UV._sort(x, dx, False)[0], torch.sort(x, dim=0).values.T)
        _line(f"d3p_sort_columns, {shape}", t_s, {"reps": n_s, "torch_sort_over_this": round(t_ts[0] / t_s[0], 2), "this_over_floor": round(t_s[0] / floor, 2),
                                                  "workspace_bytes": int(L.load().d3p_sort_columns_workspace(n, d, 0))})
        _line(f"torch.sort(x, dim=0), {shape}", t_ts, {})
        _line(f"d3p_sort_columns with ranks2, {shape}", t_r, {"torch_over_this": round(t_tr[0] / t_r[0], 2)})
        _line(f"torch.sort + 2 searchsorted, {shape}", t_tr, {})
        _line(f"cdf_distance (two sorts + d3p_column_cdf_distance), {shape}", t_c, {"torch_over_this": round(t_tc[0] / t_c[0], 2)})
        _line(f"torch composition of KS and W1, {shape}", t_tc, {})
        del x, y
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
    run(a.reps, a.side_limit, [int(s) for s in a.shapes.split(",")], bw)


if __name__ == "__main__":
    main()
