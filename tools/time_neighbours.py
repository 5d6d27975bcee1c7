#!/usr/bin/env python3
"""Times the k-nearest-neighbour entry (d3p_pair_knn, d3p_amd.neighbours) with device events after three warm-ups (developer tool).

    python tools/time_neighbours.py [--reps 9] [--side-limit 20] [--shapes 0,1,2,3]

A float32 table of n rows against a second one of the same shape, at
  0  the mixture example's shape   d = 2,     2048 rows
  1  a low-dimensional table       d = 2,    10000 rows
  2  a table of 100 000 rows       d = 64,  100000 rows
  3  images                        d = 784,  60000 rows
ALTERNATING in one process: d3p_pair_stats (the same walk without a selection: the ratio to it is the price of the selection), knn at
k = 1, 5 and 16 under the form the rule takes, knn at k = 5 with radii (the ball counts), the torch composition where its n x n matrix
would fit 1 GiB (torch.cdist without the Gram form in row batches, then topk), and prdc(k = 5) end to end (four walks and the closing reductions).

Every side runs under its own time limit: once its measured repetitions add up to --side-limit seconds it takes no further turn, and
its line reports the repetitions it got (0: the mean of its warm-ups stands in).  Per line: microseconds (median, minimum and maximum
over the repetitions), the ratio to d3p_pair_stats and the pair-columns per second.  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import fidelity as F  # noqa: E402
from d3p_amd import neighbours as N  # noqa: E402
from tools.time_fidelity import PAIR_BUDGET, _line, _time_sides  # noqa: E402

SHAPES = (("mixture example", 2, 2048), ("low-dimensional", 2, 10000), ("100 000 rows", 64, 100000), ("images", 784, 60000))
MATRIX_LIMIT = 1 << 30   # bytes of the composition's n x n float32 matrix


def _torch_knn(a, b, k):
    """The composition: row batches of the distance matrix without the Gram form (time_fidelity's: at most 2^22 pairs per call), topk."""
    batch = max(1, PAIR_BUDGET // b.shape[0])
    parts = [torch.topk(torch.cdist(a[lo:lo + batch], b, compute_mode="donot_use_mm_for_euclid_dist"), k, dim=1, largest=False)
             for lo in range(0, a.shape[0], batch)]
    return torch.cat([p.values for p in parts]), torch.cat([p.indices for p in parts])


def run(reps, limit_s, which):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    for idx in which:
        name, d, n = SHAPES[idx]
        a, b = torch.randn((n, d), device="cuda", generator=g), torch.randn((n, d), device="cuda", generator=g)
        dims = (n, d, d)
        rad = N._walk(b, dims, b, dims, 5, True, None)["sq"][:, 4].contiguous()
        sides = [("d3p_pair_stats", lambda: F._walk(a, dims, b, dims, False))]
        sides += [(f"d3p_pair_knn k={k}", lambda k=k: N._walk(a, dims, b, dims, k, False, None)) for k in (1, 5, 16)]
        sides += [("d3p_pair_knn k=5 with radii", lambda: N._walk(a, dims, b, dims, 5, False, rad)), ("prdc k=5, four walks", lambda: N.prdc(a, b, 5))]
        fits = 4 * n * n <= MATRIX_LIMIT
        if fits:
            sides.append(("torch.cdist (no Gram form) + topk k=5", lambda: _torch_knn(a, b, 5)))
        times = _time_sides([fn for _, fn in sides], reps, limit_s)
        shape = f"{name}: d={d} {n} x {n} float32"
        base = times[0][0][0]
        for (label, _), (t, got) in zip(sides, times):
            _line(f"{label}, {shape}", t, {"reps": got, "over_pair_stats": round(t[0] / base, 3),
                                          "pair_columns_per_s": round(n * n * d / (t[0] * 1e-6)) if "prdc" not in label else None,
                                          "form": int(lib.d3p_pair_knn_form(n, n, d, 5)), "workspace_bytes": int(lib.d3p_pair_knn_workspace(n, n, d, 5))})
        if fits:
            ours, ref = N._walk(a, dims, b, dims, 5, False, None), _torch_knn(a, b, 5)
            print(f"    index differs from the composition's in {int((ours['index'] != ref[1]).sum())} of {5 * n} places, largest distance "
                  f"difference {float((ours['distance'] - ref[0]).abs().max()):.3g}")
        del a, b, rad
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--side-limit", type=float, default=20.0, help="seconds of measured time after which a side takes no further turn")
    ap.add_argument("--shapes", default="0,1,2,3", help="comma-separated indices of the shapes to run")
    a = ap.parse_args()
    L.require_device()
    run(a.reps, a.side_limit, [int(s) for s in a.shapes.split(",")])


if __name__ == "__main__":
    main()
