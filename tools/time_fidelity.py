#!/usr/bin/env python3
"""Times the pair-statistics entry (d3p_pair_stats, d3p_amd.fidelity) with device events after three warm-ups (developer tool).

    python tools/time_fidelity.py [--reps 21] [--side-limit 20] [--shapes 0,1,2,3]

d3p_pair_stats alone on two resident tables, at
  0  the mixture example's shape   d = 2,    2048 x  2048 (float32)
  1  BASELINE config 3's shape     d = 64,   8192 x  8192 (float32)
  2  a table of 65 536 rows        d = 64,  65536 x 65536 (float32)
  3  VAE-like images               d = 784,  4096 x  4096 (int32 in {0, 1})
under the form the entry's rule takes and under each forced form, ALTERNATING in one process with the torch composition on the same
tables: torch.cdist per batch of rows with compute_mode="donot_use_mm_for_euclid_dist" (the Gram form would not keep the error bound;
at most 2^22 pairs per call, so the n_a x n_b matrix never exists whole), plus the float64 sum and the min / argmin of every row.

Every side runs under its own time limit: once its measured repetitions add up to --side-limit seconds it takes no further turn, and
its line reports the repetitions it got (0: the mean of its warm-ups stands in).  Per line: microseconds (median, minimum and maximum
over the repetitions), the ratio of the medians, the pair-columns per second, and the largest differences of the entry's outputs from
the composition's.  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import fidelity as F  # noqa: E402
from tools.time_waic import _event_us, _line, _stats  # noqa: E402

SHAPES = (("mixture example", 2, 2048, 2048, torch.float32), ("config 3", 64, 8192, 8192, torch.float32),
          ("65 536 rows", 64, 65536, 65536, torch.float32), ("VAE-like", 784, 4096, 4096, torch.int32))
PAIR_BUDGET = 1 << 22   # na-batch x nb per cdist call: its kernel takes one workgroup per output element and the grid is finite


def _torch_stats(a, b):
    """The composition: row batches of the distance matrix without the Gram form, reduced in float64 / by min."""
    na, nb = a.shape[0], b.shape[0]
    s = torch.empty(na, dtype=torch.float64, device=a.device)
    m = torch.empty(na, dtype=torch.float32, device=a.device)
    am = torch.empty(na, dtype=torch.int64, device=a.device)
    bf = b.float()
    batch = max(1, PAIR_BUDGET // nb)
    for lo in range(0, na, batch):
        dist = torch.cdist(a[lo:lo + batch].float(), bf, compute_mode="donot_use_mm_for_euclid_dist")
        s[lo:lo + batch] = dist.double().sum(dim=1)
        m[lo:lo + batch], am[lo:lo + batch] = dist.min(dim=1)
    return s, m, am


def _time_sides(fns, reps, limit_s, warmup=3):
    """Every side once per repetition, in turn, after `warmup` turns each; a side whose measured time has reached limit_s (its warm-ups
    counted) takes no further turn: [((median, min, max), repetitions)]."""
    spent, runs = [0.0] * len(fns), [0] * len(fns)
    ts = [[] for _ in fns]
    for k in range(warmup + reps):
        for i, fn in enumerate(fns):
            if spent[i] >= limit_s * 1e6:
                continue
            us = _event_us(fn)
            spent[i] += us
            runs[i] += 1
            if k >= warmup:
                ts[i].append(us)
    # (a side whose warm-ups alone used its limit up: their mean stands in, reported with 0 repetitions)
    return [(_stats(t), len(t)) if t else ((spent[i] / runs[i],) * 3, 0) for i, t in enumerate(ts)]


def kernel_alone(reps, limit_s, which):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    for idx in which:
        name, d, na, nb, dtype = SHAPES[idx]
        if dtype == torch.int32:
            a = torch.randint(0, 2, (na, d), device="cuda", generator=g, dtype=torch.int32)
            b = torch.randint(0, 2, (nb, d), device="cuda", generator=g, dtype=torch.int32)
        else:
            a = torch.randn((na, d), device="cuda", generator=g)
            b = torch.randn((nb, d), device="cuda", generator=g)
        da, db = (na, d, d), (nb, d, d)

        def forced(form):
            def run():
                lib.d3p_pair_stats_set_form(form)
                F._walk(a, da, b, db, False)
                lib.d3p_pair_stats_set_form(0)
            return run
        rule = int(lib.d3p_pair_stats_form(na, nb, d))
        (t_rule, n_rule), (t_wide, n_wide), (t_split, n_split), (t_torch, n_torch) = _time_sides(
            [forced(0), forced(1), forced(2), lambda: _torch_stats(a, b)], reps, limit_s)
        got, ref = F._walk(a, da, b, db, False), _torch_stats(a, b)
        shape = f"{name}: d={d} {na} x {nb} {str(dtype).replace('torch.', '')}"
        _line(f"d3p_pair_stats, the rule's form ({rule}), {shape}", t_rule,
              {"reps": n_rule, "pair_columns_per_s": round(na * nb * d / (t_rule[0] * 1e-6)), "torch_over_this": round(t_torch[0] / t_rule[0], 2),
               "max_rel_sum_diff_vs_torch": float(((got["sum"] - ref[0]).abs() / ref[0]).max()),
               "max_abs_min_diff_vs_torch": float((got["min"] - ref[1]).abs().max()),
               "argmin_differs_in": int((got["argmin"] != ref[2]).sum())})
        _line(f"d3p_pair_stats, wide form (1), {shape}", t_wide, {"reps": n_wide})
        _line(f"d3p_pair_stats, split form (2), {shape}", t_split,
              {"reps": n_split, "workspace_bytes": -(-nb // (lib.d3p_pair_stats_tile_rows() * lib.d3p_pair_stats_segment_tiles())) * na * 20})
        _line(f"torch.cdist (no Gram form) in row batches + float64 sum + min, {shape}", t_torch, {"reps": n_torch})
        del a, b, got, ref
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--side-limit", type=float, default=20.0, help="seconds of measured time after which a side takes no further turn")
    ap.add_argument("--shapes", default="0,1,2,3", help="comma-separated indices of the shapes to run")
    a = ap.parse_args()
    L.require_device()
    kernel_alone(a.reps, a.side_limit, [int(s) for s in a.shapes.split(",")])


if __name__ == "__main__":
    main()
