#!/usr/bin/env python3
"""Times d3p_amd.predictive.predictive_samples for the linear and Poisson families with device events after a warm-up (developer
tool).

    python tools/time_predictive_glm.py [--reps 20]

Cases: 10^6 rows, d = 512 + intercept, 128 draws, and the reference example's shape (d = 4, 10^4 rows, 100 draws).  Per case and
family the outcome kernel (k_predict_glm), the logistic predictive kernel (k_predict_logreg: the same tile and grid, a Bernoulli
epilogue) at the same shape, timed before and after it -- the difference of its two medians is the run-to-run spread the comparison
has to allow for -- and a torch composition of the same work: X @ W.T + b, then torch.normal / torch.poisson.  Per line: microseconds
(median, minimum and maximum over the repetitions), FLOP/s of the product and its fraction of the 157.3 TFLOP/s fp32 rate, the
algorithmic bytes (X read once, the latent rows, the n x rows outcomes written) over the time.  The samples are given as one packed
buffer, so nothing is copied before the launch; the key split is inside the timed call in both kernels' lines.
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
import d3p_amd.random.debug as jr  # noqa: E402
from d3p_amd import infer_util as U  # noqa: E402
from d3p_amd import predictive as Ps  # noqa: E402
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


def _torch_outcomes(family, W, b, X):
    t = torch.matmul(W, X.T) + b[:, None]
    if family == "linear":
        return torch.normal(t, SIGMA)
    return torch.poisson(torch.exp(t))


def cases(reps):
    key = jr.PRNGKey(0)
    for d, rows, n in ((512, 1_000_000, 128), (4, 10_000, 100)):
        g = torch.Generator(device="cuda").manual_seed(0)
        # features N(0, 1) / sqrt(d) and draws of norm about 1: rates around 1 with a tail on both sides of the rule's threshold of 10
        X = torch.randn((rows, d), device="cuda", generator=g) / math.sqrt(d)
        lat = torch.randn((n, d + 1), device="cuda", generator=g) / math.sqrt(d)
        lat[:, d] += 1.5
        s = {"w": lat[:, :d], "intercept": lat[:, d]}
        assert U._packed_view(s["w"], s["intercept"], n, d) is not None
        W, b = lat[:, :d].contiguous(), lat[:, d].contiguous()
        logi = LogisticRegression(d, intercept=True)
        flop = 2 * n * rows * d
        nbytes = rows * d * 4 + n * (d + 1) * 4 + n * rows * 4
        for family in ("linear", "poisson"):
            model = LinearRegression(d, intercept=True, obs_scale=SIGMA) if family == "linear" else PoissonRegression(d, intercept=True)
            shape = f"{family} d={d} rows={rows} n={n}"
            t_log_a = _time(lambda: Ps.predictive_samples(key, logi, s, X), reps)
            t_glm = _time(lambda: Ps.predictive_samples(key, model, s, X), reps)
            t_log_b = _time(lambda: Ps.predictive_samples(key, logi, s, X), reps)
            t_comp = _time(lambda: _torch_outcomes(family, W, b, X), max(3, reps // 2))
            spread = abs(t_log_a[0] - t_log_b[0])
            _line(f"logistic predictive (before) {shape}", t_log_a, flop, nbytes)
            _line(f"predictive_samples {shape}", t_glm, flop, nbytes,
                  {"speedup_over_torch": round(t_comp[0] / t_glm[0], 2), "over_logistic": round(t_glm[0] / min(t_log_a[0], t_log_b[0]), 3),
                   "logistic_run_to_run_us": round(spread, 1)})
            _line(f"logistic predictive (after) {shape}", t_log_b, flop, nbytes)
            _line(f"torch composition {shape}", t_comp, flop, nbytes + 2 * n * rows * 4)
            got, ref = Ps.predictive_samples(key, model, s, X).double(), _torch_outcomes(family, W, b, X).double()
            print(json.dumps({"case": f"outcome means, kernel against the torch composition {shape}", "kernel": float(got.mean()),
                              "torch": float(ref.mean())}), flush=True)
            del got, ref
        del X, lat, W, b
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    L.require_device()
    cases(args.reps)


if __name__ == "__main__":
    main()
