#!/usr/bin/env python3
"""Times the label-sums entry (d3p_pair_label_sums, d3p_amd.permutation) with device events after three warm-ups (developer tool).

    python tools/time_permutation.py [--reps 21] [--side-limit 20] [--shapes 0,1,2]

d3p_pair_label_sums alone on a resident pooled table, resident labels and resident row sums, at
  0  the mixture example's shape   d = 2,    4096 pooled rows, 1000 labellings (float32)
  1  BASELINE config 3's shape     d = 64,  16384 pooled rows, 1000 labellings (float32)
  2  VAE-like images               d = 784,  4096 pooled rows,  200 labellings (int32 in {0, 1})
ALTERNATING in one process with d3p_pair_stats of the table against itself at that shape (the same distances without the labellings:
what is left of the entry's time is its phase 2) and with the torch composition: torch.cdist without the Gram form in row batches,
widened to float64, and G^T D G's diagonal as ((D @ G) * G).sum(0) for the 0/1 matrix G of the labellings.

Every side runs under its own time limit: once its measured repetitions add up to --side-limit seconds it takes no further turn, and
its line reports the repetitions it got (0: the mean of its warm-ups stands in).  Per line: microseconds (median, minimum and maximum
over the repetitions), the ratios of the medians, the pair-labellings per second, and the largest relative difference of s11 from the
composition's.  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import fidelity as F  # noqa: E402
from d3p_amd import permutation as P  # noqa: E402
from tools.time_fidelity import PAIR_BUDGET, _time_sides  # noqa: E402
from tools.time_waic import _line  # noqa: E402

SHAPES = (("mixture example", 2, 4096, 1000, torch.float32), ("config 3", 64, 16384, 1000, torch.float32),
          ("VAE-like", 784, 4096, 200, torch.int32))
MATRIX_ROWS = 16384   # the composition's m x R float64 matrix G and its products: taken up to this many rows


def _torch_sums(z, G):
    """The composition: row batches of the distance matrix without the Gram form (at most 2^22 pairs per cdist call, as
    tools/time_fidelity.py), widened to float64, and the quadratic form of every labelling."""
    zf = z.float()
    m = zf.shape[0]
    batch = max(1, PAIR_BUDGET // m)
    s = torch.zeros(G.shape[1], dtype=torch.float64, device=z.device)
    for lo in range(0, m, batch):
        D = torch.cdist(zf[lo:lo + batch], zf, compute_mode="donot_use_mm_for_euclid_dist").double()
        s += ((D @ G) * G[lo:lo + batch]).sum(dim=0)
    return s


def kernel_alone(reps, limit_s, which):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    for idx in which:
        name, d, m, R, dtype = SHAPES[idx]
        if dtype == torch.int32:
            z = torch.randint(0, 2, (m, d), device="cuda", generator=g, dtype=torch.int32)
        else:
            z = torch.randn((m, d), device="cuda", generator=g)
        dz = (m, d, d)
        labels = P.permutation_labels(m // 2, m - m // 2, R - 1, seed=0, device="cuda")
        row_sum = F._walk(z, dz, z, dz, True)["sum"]
        sides = [lambda: P._sums(z, dz, labels, R, row_sum), lambda: F._walk(z, dz, z, dz, True)]
        G = None
        if m <= MATRIX_ROWS:
            bits = (labels.view(torch.int32).to(torch.int64)[:, :, None] >> torch.arange(32, device="cuda")) & 1      # (tiles, R, 32)
            G = bits.permute(0, 2, 1).reshape(-1, R)[:m].double()
            sides.append(lambda: _torch_sums(z, G))
        times = _time_sides(sides, reps, limit_s)
        (t_this, n_this), (t_pairs, n_pairs) = times[0], times[1]
        shape = f"{name}: d={d} {m} pooled rows, {R} labellings, {str(dtype).replace('torch.', '')}"
        extra = {"reps": n_this, "pair_labellings_per_s": round(m * m * R / (t_this[0] * 1e-6)), "pair_stats_share": round(t_pairs[0] / t_this[0], 3),
                 "workspace_bytes": int(lib.d3p_pair_label_sums_workspace(m, d, R))}
        if G is not None:
            got, ref = P._sums(z, dz, labels, R, row_sum)[0], _torch_sums(z, G)
            extra.update({"torch_over_this": round(times[2][0][0] / t_this[0], 2), "max_rel_s11_diff_vs_torch": float(((got - ref).abs() / ref).max())})
        _line(f"d3p_pair_label_sums, {shape}", t_this, extra)
        _line(f"d3p_pair_stats of the table against itself, {shape}", t_pairs, {"reps": n_pairs})
        if G is not None:
            _line(f"torch.cdist (no Gram form) -> float64, ((D @ G) * G).sum(0), {shape}", times[2][0], {"reps": times[2][1]})
        del z, labels, row_sum, G
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--side-limit", type=float, default=20.0, help="seconds of measured time after which a side takes no further turn")
    ap.add_argument("--shapes", default="0,1,2", help="comma-separated indices of the shapes to run")
    a = ap.parse_args()
    L.require_device()
    kernel_alone(a.reps, a.side_limit, [int(s) for s in a.shapes.split(",")])


if __name__ == "__main__":
    main()
