#!/usr/bin/env python3
"""Times d3p_amd.prediction.predictive_moments with device events after a warm-up (developer tool).

    python tools/time_moments.py [--reps 20]

Cases, for the three regression families: 10^6 rows, d = 512 + intercept, 128 draws, and the reference example's shape (d = 4, 10^4
rows, 100 draws).  Per case the moments kernel, the lppd form of d3p_amd.infer_util on the same inputs (the same product loop, an
epilogue at least as heavy for the logistic and Poisson families) and a torch composition of the same work: X @ W.T + b, the link,
mean / var over the draws.  Per line: microseconds (median, minimum and maximum over the repetitions), FLOP/s of the product and its
fraction of the 157.3 TFLOP/s fp32 rate, the algorithmic bytes (X read once, the latent rows, the outputs written) over the time.
The lppd form is timed twice, before and after the moments kernel: the difference of its two medians is the run-to-run spread the
comparison has to allow for.  The samples are given as one packed buffer, so nothing is copied before the launch.
Fails without a GPU (no fallback)."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
from d3p_amd import infer_util as U  # noqa: E402
from d3p_amd import prediction as Pm  # noqa: E402
from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression  # noqa: E402

FP32_PEAK = 157.3e12
SIGMA = 0.5


def _time(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def _line(name, us, flop, nbytes, extra=None):
    rec = {"case": name, "us_median": round(us[0], 1), "us_min": round(us[1], 1), "us_max": round(us[2], 1), "flop": flop,
           "tflops": round(flop / (us[0] * 1e-6) / 1e12, 2), "fp32_fraction": round(flop / (us[0] * 1e-6) / FP32_PEAK, 3),
           "bytes": nbytes, "TB_per_s": round(nbytes / (us[0] * 1e-6) / 1e12, 3)}
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)
    return rec


def _problem(family, d, rows, n):
    """Features N(0, 1) / sqrt(d) and draws of norm about 1, so that the linear predictor stays in a range every family evaluates."""
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.randn((rows, d), device="cuda", generator=g) / math.sqrt(d)
    lat = torch.randn((n, d + 1), device="cuda", generator=g) / math.sqrt(d)
    if family == "logistic":
        y = (torch.rand(rows, device="cuda", generator=g) < 0.5).float()
        model = LogisticRegression(d, intercept=True)
    elif family == "linear":
        y = torch.randn(rows, device="cuda", generator=g)
        model = LinearRegression(d, intercept=True, obs_scale=SIGMA)
    else:
        y = torch.poisson(torch.ones(rows, device="cuda"), generator=g)
        model = PoissonRegression(d, intercept=True)
    return model, X, y, lat


def _torch_moments(family, W, b, X):
    t = torch.matmul(W, X.T) + b[:, None]
    if family == "logistic":
        mu = torch.sigmoid(t)
        v = mu * (1.0 - mu)
    elif family == "linear":
        mu, v = t, None
    else:
        mu = torch.exp(t)
        v = mu
    within = v.mean(dim=0) if v is not None else SIGMA * SIGMA
    return mu.mean(dim=0), within + mu.var(dim=0, unbiased=False)


def cases(reps):
    out = []
    for d, rows, n in ((512, 1_000_000, 128), (4, 10_000, 100)):
        for family in ("logistic", "linear", "poisson"):
            model, X, y, lat = _problem(family, d, rows, n)
            s = {"w": lat[:, :d], "intercept": lat[:, d]}
            assert U._packed_view(s["w"], s["intercept"], n, d) is not None
            flop = 2 * n * rows * d
            read = rows * d * 4 + n * (d + 1) * 4
            shape = f"{family} d={d} rows={rows} n={n}"
            t_lppd_a = _time(lambda: U.log_predictive_density(model, s, X, y), reps)
            t_mom = _time(lambda: Pm.predictive_moments(model, s, X), reps)
            t_lppd_b = _time(lambda: U.log_predictive_density(model, s, X, y), reps)
            W, b = lat[:, :d].contiguous(), lat[:, d].contiguous()
            t_comp = _time(lambda: _torch_moments(family, W, b, X), max(3, reps // 2))
            spread = abs(t_lppd_a[0] - t_lppd_b[0])
            out.append(_line(f"lppd form (before) {shape}", t_lppd_a, flop, read + rows * 8))
            out.append(_line(f"moments {shape}", t_mom, flop, read + rows * 8,
                             {"speedup_over_torch": round(t_comp[0] / t_mom[0], 2), "over_lppd": round(t_mom[0] / min(t_lppd_a[0], t_lppd_b[0]), 3),
                              "lppd_run_to_run_us": round(spread, 1),
                              "within_lppd_plus_spread": bool(t_mom[0] <= max(t_lppd_a[0], t_lppd_b[0]) + spread)}))
            out.append(_line(f"lppd form (after) {shape}", t_lppd_b, flop, read + rows * 8))
            out.append(_line(f"torch composition {shape}", t_comp, flop, read + rows * 8 + 4 * n * rows * 4))
            got, ref = Pm.predictive_moments(model, s, X), _torch_moments(family, W, b, X)      # the two compute the same thing
            print(json.dumps({"case": f"moments against the torch composition {shape}",
                              "max_abs_difference_mean": float((got["mean"] - ref[0]).abs().max()),
                              "max_abs_difference_variance": float((got["variance"] - ref[1]).abs().max())}), flush=True)
            del X, y, lat, W, b, got, ref
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    L.require_device()
    cases(args.reps)


if __name__ == "__main__":
    main()
