#!/usr/bin/env python3
"""Times the mixed-type pair statistics (d3p_pair_stats_mixed, d3p_amd.mixed), pack launches included, with device events (developer tool).

    python tools/time_mixed.py [--reps 7] [--warmup 2] [--side-limit 20] [--shapes 0,1,2]

The entry on two resident float32 tables, at
  0  d = 64: 32 numeric + 32 categorical columns   100000 x 100000
  1  d = 128, all categorical                      100000 x 100000
  2  d = 2: one numeric + one categorical column    10000 x  10000
ALTERNATING in one process with d3p_pair_stats (the Euclidean walk) on a float32 table of the same d and rows, and with the torch
composition: torch.cdist(p=1) on the scaled numeric part plus a compare-and-sum on the codes, per batch of rows (at most 2^22 pairs a
call), reduced to the float64 sum and the min / argmin of every row.  Every side runs under its own time limit (tools/time_fidelity.py).
Per line: microseconds (median, minimum, maximum), the ratios of the medians and the largest differences from the composition.  Fails
without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import fidelity as F  # noqa: E402
from d3p_amd import mixed as M  # noqa: E402
from tools.time_fidelity import PAIR_BUDGET, _time_sides  # noqa: E402
from tools.time_waic import _line  # noqa: E402

SHAPES = (("32 numeric + 32 categorical", 32, 32, 100000), ("all categorical", 0, 128, 100000), ("1 numeric + 1 categorical", 1, 1, 10000))


def _torch_stats(a, b, dn, scale, w_cat):
    na, nb = a.shape[0], b.shape[0]
    s = torch.empty(na, dtype=torch.float64, device=a.device)
    m = torch.empty(na, dtype=torch.float32, device=a.device)
    am = torch.empty(na, dtype=torch.int64, device=a.device)
    bn, bc = b[:, :dn] * scale, b[:, dn:].to(torch.uint8)
    batch = max(1, PAIR_BUDGET // nb)
    for lo in range(0, na, batch):
        dist = torch.zeros((min(batch, na - lo), nb), device=a.device)
        if dn:
            dist += torch.cdist(a[lo:lo + batch, :dn] * scale, bn, p=1)
        if dn < a.shape[1]:
            ac = a[lo:lo + batch, dn:].to(torch.uint8)
            for c in range(ac.shape[1]):                                     # (a column at a time: no batch x nb x dc tensor)
                dist += w_cat * (ac[:, c, None] != bc[None, :, c])
        s[lo:lo + batch] = dist.double().sum(dim=1)
        m[lo:lo + batch], am[lo:lo + batch] = dist.min(dim=1)
    return s, m, am


def run(reps, warmup, limit_s, which):
    g = torch.Generator(device="cuda").manual_seed(0)
    for idx in which:
        name, dn, dc, n = SHAPES[idx]
        d = dn + dc
        tabs = []
        for _ in range(2):
            t = torch.randn((n, d), device="cuda", generator=g)
            t[:, dn:] = torch.randint(0, 8, (n, dc), device="cuda", generator=g).float()
            tabs.append(t)
        a, b = tabs
        schema = M.mixed_schema(b, tuple(range(dn, d)))
        scale = torch.tensor(schema.scale[:dn], device="cuda")
        dims = (n, d, d)
        (t_mix, n_mix), (t_euc, n_euc), (t_torch, n_torch) = _time_sides(
            [lambda: M._walk(a, dims, b, dims, False, schema), lambda: F._walk(a, dims, b, dims, False),
             lambda: _torch_stats(a, b, dn, scale, schema.w_cat)], reps, limit_s, warmup)
        got, ref = M._walk(a, dims, b, dims, False, schema), _torch_stats(a, b, dn, scale, schema.w_cat)
        shape = f"{name}: d={d} {n} x {n} float32"
        _line(f"d3p_pair_stats_mixed with its pack launches, {shape}", t_mix,
              {"reps": n_mix, "pairs_per_s": round(n * n / (t_mix[0] * 1e-6)), "euclidean_over_this": round(t_euc[0] / t_mix[0], 2),
               "torch_over_this": round(t_torch[0] / t_mix[0], 2),
               "max_rel_sum_diff_vs_torch": float(((got["sum"] * schema.total_weight - ref[0]).abs() / ref[0]).max()),
               "max_abs_min_diff_vs_torch": float((got["min"] * schema.total_weight - ref[1]).abs().max())})
        _line(f"d3p_pair_stats (Euclidean, the same d and rows), {shape}", t_euc, {"reps": n_euc})
        _line(f"torch.cdist(p=1) + compare-and-sum in row batches + float64 sum + min, {shape}", t_torch, {"reps": n_torch})
        del a, b, tabs, got, ref
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--side-limit", type=float, default=20.0, help="seconds of measured time after which a side takes no further turn")
    ap.add_argument("--shapes", default="0,1,2", help="comma-separated indices of the shapes to run")
    a = ap.parse_args()
    L.require_device()
    run(a.reps, a.warmup, a.side_limit, [int(s) for s in a.shapes.split(",")])


if __name__ == "__main__":
    main()
