#!/usr/bin/env python3
"""Times the energy-score entry (d3p_energy_score, d3p_amd.energy) with device events after three warm-ups (developer tool).

    python tools/time_energy.py [--reps 21]

d3p_energy_score alone on a resident (draws, rows, d) tensor against random observations, at
  the mixture example's shape            d = 2,   2048 rows, 100 draws (float32)
  BASELINE config 3's shape              d = 64,  8192 rows, 128 draws (float32)
  a VAE-like image tensor                d = 784,  512 rows,  64 draws (int32 in {0, 1})
  many short rows (the rows form's case) d = 2,  65536 rows, 100 draws (float32)
under the form the entry's rule takes and under each forced form, ALTERNATING in one process with the torch composition on the same
tensor: torch.cdist per batch of rows with compute_mode="donot_use_mm_for_euclid_dist" (the Gram form would not keep the error bound),
plus the float64 sums (at most 2^22 pairs per call).

Per line: microseconds (median, minimum and maximum over the repetitions), the ratio of the medians, the bytes of one read of the
tensor, and the largest difference of the entry's score from the composition's.  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import energy as E  # noqa: E402
from tools.time_waic import _line, _time_alternating  # noqa: E402

SHAPES = (("mixture example", 2, 2048, 100, torch.float32), ("config 3", 64, 8192, 128, torch.float32), ("VAE-like", 784, 512, 64, torch.int32),
          ("many short rows", 2, 65536, 100, torch.float32))
PAIR_BUDGET = 1 << 22   # rows x n x n per cdist call: its kernel takes one workgroup per output element and the grid is finite


def _torch_scores(z, y):
    """The composition: (rows, n, n) and (rows, n, 1) distances without the Gram form, summed in float64."""
    n, rows, d = z.shape
    es = torch.empty(rows, dtype=torch.float64, device=z.device)
    batch = max(1, PAIR_BUDGET // (n * n))
    for lo in range(0, rows, batch):
        x = z[:, lo:lo + batch].permute(1, 0, 2).float()
        yy = y[lo:lo + batch].float()[:, None, :]
        s1 = torch.cdist(x, yy, compute_mode="donot_use_mm_for_euclid_dist").double().sum(dim=(1, 2))
        s2 = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist").double().sum(dim=(1, 2))
        es[lo:lo + batch] = s1 / n - s2 / (2.0 * n * n)
    return es


def kernel_alone(reps):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, d, rows, n, dtype in SHAPES:
        if dtype == torch.int32:
            z = torch.randint(0, 2, (n, rows, d), device="cuda", generator=g, dtype=torch.int32)
            y = torch.randint(0, 2, (rows, d), device="cuda", generator=g, dtype=torch.int32)
        else:
            z = torch.randn((n, rows, d), device="cuda", generator=g)
            y = torch.randn((rows, d), device="cuda", generator=g)
        dims = (n, rows, d, rows * d, d)
        yf = y.reshape(-1)

        def forced(form):
            def run():
                lib.d3p_energy_score_set_form(form)
                E._score(z, dims, yf)
                lib.d3p_energy_score_set_form(0)
            return run
        rule = int(lib.d3p_energy_score_form(n, rows, d))
        t_rule, t_rows, t_stream, t_torch = _time_alternating([forced(0), forced(1), forced(2), lambda: _torch_scores(z, y)], reps)
        got, ref = E._score(z, dims, yf)["es"].double(), _torch_scores(z, y)
        shape = f"{name}: d={d} rows={rows} draws={n} {str(dtype).replace('torch.', '')}"
        _line(f"d3p_energy_score, the rule's form ({rule}), {shape}", t_rule,
              {"rows_per_s": round(rows / (t_rule[0] * 1e-6)), "tensor_bytes": 4 * n * rows * d, "torch_over_this": round(t_torch[0] / t_rule[0], 2),
               "max_abs_es_diff_vs_torch": float((got - ref).abs().max())})
        _line(f"d3p_energy_score, rows form (1), {shape}", t_rows)
        _line(f"d3p_energy_score, streamed form (2), {shape}", t_stream)
        _line(f"torch.cdist (no Gram form) + float64 sums, {shape}", t_torch)
        del z, y, got, ref
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    L.require_device()
    kernel_alone(a.reps)


if __name__ == "__main__":
    main()
