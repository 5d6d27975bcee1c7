#!/usr/bin/env python3
"""Times the highest-density intervals (d3p_col_hpdi, d3p_amd.intervals.hpdi, kind="hpdi") with device events after a warm-up
(developer tool).

    python tools/time_hpdi.py [--reps 20] [--small]

  (a) d3p_col_hpdi alone on one resident 64 MiB slab of random normal values at L = int(0.9 n): 128 draws x 131072 columns and 1024
      draws x 16384 columns (the 32-column form), 4096 x 4096 (the 8-column form) and 16384 x 1024 (the 2-column form), each
      ALTERNATING on the same slab with the torch composition -- torch.sort(dim=0), one subtraction of two slices, argmin, two gathers
      -- and with d3p_col_quantiles at the probabilities (0.05, 0.5, 0.95);
  (b) per family at d = 512 + intercept, 10^6 rows, 128 draws and at the examples' d = 4, 10^4 rows, 100 draws (--small: the latter
      only), on latents prepared beforehand: credible_interval(kind="hpdi") against credible_interval(kind="equal_tailed"), alternating.

Per line: microseconds (median, minimum and maximum over the repetitions) and the ratios of the medians.  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import intervals as IV  # noqa: E402
from tools.time_loglik import _problem  # noqa: E402
from tools.time_waic import _line, _time_alternating  # noqa: E402

SLAB = 64 << 20
PROBS = (0.05, 0.5, 0.95)


def _torch_hpdi(m, Lq):
    """The composition: one sort over the draws, the lengths of all windows, the first minimum, the two ends."""
    s = torch.sort(m, dim=0).values
    n = m.shape[0]
    i = torch.argmin(s[Lq:] - s[:n - Lq], dim=0, keepdim=True)
    return torch.cat([torch.gather(s, 0, i), torch.gather(s, 0, i + Lq)])


def kernel_alone(reps):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (128, 1024, 4096, 16384):
        count = SLAB // (4 * n)
        buf = torch.randn((n, count), device="cuda", generator=g)
        out, q = torch.empty((2, count), device="cuda"), torch.empty((len(PROBS), count), device="cuda")
        lens = IV.window_lengths((0.9,), n)
        hd, et = IV._highest_density((0.9,)), IV._equal_tailed(PROBS)
        hd_args, et_args = hd.args(n), et.args(n)
        t_h, t_t, t_q = _time_alternating([lambda: hd.reduce(buf, torch.float32, count, n, count, hd_args, out, count),
                                           lambda: _torch_hpdi(buf, lens[0]),
                                           lambda: et.reduce(buf, torch.float32, count, n, count, et_args, q, count)], reps)
        same = bool(torch.equal(out, _torch_hpdi(buf, lens[0])))      # (continuous values: argmin's tie rule is not exercised)
        form = int(lib.d3p_col_hpdi_cols_per_group(n))
        _line(f"d3p_col_hpdi alone ({form}-column form), n={n} cols={count} L={lens[0]}", t_h,
              {"cols_per_s": round(count / (t_h[0] * 1e-6)), "slab_bytes": 4 * n * count, "torch_over_this": round(t_t[0] / t_h[0], 2),
               "this_over_quantiles": round(t_h[0] / t_q[0], 2), "equals_torch": same})
        _line(f"torch sort + subtract + argmin + gathers, the same slab n={n} cols={count}", t_t)
        _line(f"d3p_col_quantiles Q=3, the same slab n={n} cols={count}", t_q)
        del buf
        torch.cuda.empty_cache()


def regression_cases(reps, shapes):
    for d, rows, n in shapes:
        for family in ("logistic", "linear", "poisson"):
            model, _, X, y, lat = _problem(family, d, rows, n)
            s = {"w": lat[:, :d], "intercept": lat[:, d]}
            shape = f"{family} d={d} rows={rows} n={n}"
            t_h, t_e = _time_alternating([lambda: IV.credible_interval(model, s, X, kind="hpdi"),
                                          lambda: IV.credible_interval(model, s, X, kind="equal_tailed")], reps)
            _line(f"intervals.credible_interval kind=hpdi {shape}", t_h, {"over_equal_tailed": round(t_h[0] / t_e[0], 2)})
            _line(f"intervals.credible_interval kind=equal_tailed {shape}", t_e)
            del X, y, lat
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="the examples' shape only")
    a = ap.parse_args()
    L.require_device()
    kernel_alone(a.reps)
    regression_cases(a.reps, ((4, 10_000, 100),) if a.small else ((512, 1_000_000, 128), (4, 10_000, 100)))


if __name__ == "__main__":
    main()
