#!/usr/bin/env python3
"""Times the binned-marginals entry (d3p_marginals, d3p_amd.marginals) with device events after three warm-ups (developer tool).

    python tools/time_marginals.py [--reps 21] [--side-limit 10] [--shapes 0,1,2,3]

d3p_marginals alone on a resident table, resident edges and preallocated outputs and workspace, at
  0  the mixture example's shape   2048 x 2    float32, 16 bins
  1  a million rows                10^6 x 64   float32, 16 bins, uniform codes            (2016 pairs)
  2  the same, every row equal     10^6 x 64   float32, 16 bins: all lanes on ONE cell    (the conflict case)
  3  VAE-like images               4096 x 784  int32 in {0, 1}, B = 2                    (306 936 pairs)
ALTERNATING in one process with the torch composition on the same table: torch.bucketize per column, then one
torch.bincount(ci * K + cj, minlength=K^2) per pair of columns -- d (d - 1) / 2 launches over n rows.

Every side runs under its own time limit: once its measured repetitions add up to --side-limit seconds it takes no further turn, and
its line reports the repetitions it got (0: the mean of its warm-ups stands in).  Per line: microseconds (median, minimum and maximum
over the repetitions), the ratio of the medians, the pair increments per second (n d (d - 1) / 2 over the median) and the number of
cells in which the entry's counts differ from the composition's (0).  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from tools.time_fidelity import _time_sides  # noqa: E402
from tools.time_waic import _line  # noqa: E402

SHAPES = (("mixture example", 2048, 2, 16, "float"), ("a million rows, uniform codes", 10 ** 6, 64, 16, "float"),
          ("a million rows, every row equal", 10 ** 6, 64, 16, "equal"), ("VAE-like", 4096, 784, 2, "binary"))


def _torch_counts(x, edges, B):
    """The composition: bucketize per column, one bincount per pair."""
    n, d = x.shape
    K = B + 1
    xf = x.float()
    codes = [torch.bucketize(xf[:, c].contiguous(), edges[c], right=False) for c in range(d)]
    one = torch.stack([torch.bincount(c, minlength=K) for c in codes])
    two = [torch.bincount(codes[i] * K + codes[j], minlength=K * K) for i in range(d) for j in range(i + 1, d)]
    return one, (torch.stack(two).reshape(-1, K, K) if two else torch.zeros((0, K, K), dtype=torch.int64, device=x.device))


def kernel_alone(reps, limit_s, which):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    for idx in which:
        name, n, d, B, kind = SHAPES[idx]
        K, P = B + 1, d * (d - 1) // 2
        if kind == "binary":
            x = torch.randint(0, 2, (n, d), device="cuda", generator=g, dtype=torch.int32)
            edges = torch.zeros((d, 1), device="cuda")
        else:
            x = torch.rand((n, d), device="cuda", generator=g) if kind == "float" else torch.full((n, d), 0.5, device="cuda")
            edges = (torch.arange(1, B, device="cuda", dtype=torch.float32) / B).repeat(d, 1).contiguous()
        nbins = torch.full((d,), B, dtype=torch.int32, device="cuda")
        one = torch.empty((d, K), dtype=torch.int32, device="cuda")
        two = torch.empty((max(P, 1), K, K), dtype=torch.int32, device="cuda")
        ws = torch.empty(int(lib.d3p_marginals_workspace(n, d, B)), dtype=torch.uint8, device="cuda")

        def run():
            L.check(lib.d3p_marginals(L.stream_ptr(), L.ptr(x), 0 if x.dtype == torch.float32 else 1, d, n, d, B, L.ptr(nbins), L.ptr(edges),
                                      L.ptr(one), L.ptr(two), L.ptr(ws), int(ws.numel())))
        (t_this, n_this), (t_torch, n_torch) = _time_sides([run, lambda: _torch_counts(x, edges, B)], reps, limit_s)
        run()
        ref = _torch_counts(x, edges, B)
        differ = int((one.to(torch.int64) != ref[0]).sum()) + int((two[:P].to(torch.int64) != ref[1]).sum())
        shape = f"{name}: {n} x {d} {str(x.dtype).replace('torch.', '')}, B = {B}, {P} pairs"
        _line(f"d3p_marginals, {shape}", t_this,
              {"reps": n_this, "pair_increments_per_s": round(n * P / (t_this[0] * 1e-6)), "torch_over_this": round(t_torch[0] / t_this[0], 2),
               "cells_differing_from_torch": differ, "workspace_bytes": int(ws.numel()), "two_way_bytes": P * K * K * 4})
        _line(f"torch.bucketize per column + torch.bincount per pair, {shape}", t_torch, {"reps": n_torch})
        del x, one, two, ws, ref
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--side-limit", type=float, default=10.0, help="seconds of measured time after which a side takes no further turn")
    ap.add_argument("--shapes", default="0,1,2,3", help="comma-separated indices of the shapes to run")
    a = ap.parse_args()
    L.require_device()
    kernel_alone(a.reps, a.side_limit, [int(s) for s in a.shapes.split(",")])


if __name__ == "__main__":
    main()
