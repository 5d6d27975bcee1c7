#!/usr/bin/env python3
"""Times the CRPS / PIT entry (d3p_col_crps, d3p_amd.scoring.score_draws) with device events after a warm-up (developer tool).

    python tools/time_scoring.py [--reps 20]

d3p_col_crps alone on one resident 64 MiB slab of random normal values against random normal observations: 128 draws x 131072 columns
and 1024 draws x 16384 columns (the 32-column form), 4096 x 4096 (the 8-column form) and 16384 x 1024 (the 2-column form), each
ALTERNATING on the same slab with
  d3p_col_hpdi at one window length L = int(0.9 n) -- the same staging and sort with a cheaper scan;
  the torch composition -- torch.sort(dim=0), one weighted sum and one absolute sum in float64, two comparisons.

Per line: microseconds (median, minimum and maximum over the repetitions), the ratios of the medians, and the largest difference of
the entry's CRPS from the composition's.  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import intervals as IV  # noqa: E402
from d3p_amd import scoring as SC  # noqa: E402
from tools.time_waic import _line, _time_alternating  # noqa: E402

SLAB = 64 << 20


def _torch_scores(m, y):
    """The composition: one sort over the draws, the two sums in float64, the two counts."""
    n = m.shape[0]
    d = torch.sort(m, dim=0).values.double() - y.double()[None, :]
    w = (2.0 * torch.arange(n, device=m.device, dtype=torch.float64) - n + 1.0)[:, None]
    crps = d.abs().sum(dim=0) / n - (w * d).sum(dim=0) / (n * n)
    return crps, (m < y[None, :]).sum(dim=0), (m == y[None, :]).sum(dim=0)


def kernel_alone(reps):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (128, 1024, 4096, 16384):
        count = SLAB // (4 * n)
        buf = torch.randn((n, count), device="cuda", generator=g)
        y = torch.randn((count,), device="cuda", generator=g)
        hd = IV._highest_density((0.9,))
        hd_args, hd_out = hd.args(n), torch.empty((2, count), device="cuda")
        t_c, t_h, t_t = _time_alternating([lambda: SC._score(buf, count, n, count, y),
                                           lambda: hd.reduce(buf, torch.float32, count, n, count, hd_args, hd_out, count),
                                           lambda: _torch_scores(buf, y)], reps)
        got, (ref, below, equal) = SC._score(buf, count, n, count, y), _torch_scores(buf, y)
        same = bool(torch.equal(got["below"].long(), below)) and bool(torch.equal(got["equal"].long(), equal))
        form = int(lib.d3p_col_crps_cols_per_group(n))
        _line(f"d3p_col_crps alone ({form}-column form), n={n} cols={count}", t_c,
              {"cols_per_s": round(count / (t_c[0] * 1e-6)), "slab_bytes": 4 * n * count, "this_over_hpdi": round(t_c[0] / t_h[0], 2),
               "torch_over_this": round(t_t[0] / t_c[0], 2), "max_abs_crps_diff_vs_torch": float((got["crps"].double() - ref).abs().max()),
               "counts_equal_torch": same})
        _line(f"d3p_col_hpdi one window length, the same slab n={n} cols={count}", t_h)
        _line(f"torch sort + float64 sums + two comparisons, the same slab n={n} cols={count}", t_t)
        del buf, y, got, ref
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    L.require_device()
    kernel_alone(a.reps)


if __name__ == "__main__":
    main()
