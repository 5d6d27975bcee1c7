#!/usr/bin/env python3
"""Times d3p_amd.infer_util (log_likelihood, log_predictive_density) with device events after a warm-up (developer tool).

    python tools/time_loglik.py [--reps 10]

Cases, for the three regression families: 10^6 rows, d = 512 + intercept, 128 draws, and the reference example's shape (d = 4, 10^4
rows, 100 draws).  Per case the rows form (the n x rows matrix is written), the lppd form (it is not) and a torch composition of the
same work: X @ W.T + b, torch.distributions' log_prob, torch.logsumexp - log n.  Per line: microseconds (median and minimum over the
repetitions), FLOP/s of the product and its fraction of the 157.3 TFLOP/s fp32 rate, the algorithmic bytes (X and y read once, the
latent rows, the output written) over the time.  The samples are given as one packed buffer, so nothing is copied before the launch.
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
from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression  # noqa: E402

FP32_PEAK = 157.3e12


def _time(fn, reps, warmup=2):
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
    return float(np.median(ts)), float(np.min(ts))


def _line(name, us, flop, nbytes, extra=None):
    rec = {"case": name, "us_median": round(us[0], 1), "us_min": round(us[1], 1), "flop": flop,
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
    t = X[:4096] @ lat[0, :d] + lat[0, d]
    if family == "logistic":
        y = (torch.rand(rows, device="cuda", generator=g) < 0.5).float()
        model, dist = LogisticRegression(d, intercept=True), lambda t_: torch.distributions.Bernoulli(logits=t_)
    elif family == "linear":
        y = torch.randn(rows, device="cuda", generator=g)
        model, dist = LinearRegression(d, intercept=True, obs_scale=0.5), lambda t_: torch.distributions.Normal(t_, 0.5)
    else:
        y = torch.poisson(torch.ones(rows, device="cuda"), generator=g)
        model, dist = PoissonRegression(d, intercept=True), lambda t_: torch.distributions.Poisson(torch.exp(t_), validate_args=False)
    assert float(t.abs().max()) < 20.0
    return model, dist, X, y, lat


def cases(reps):
    out = []
    for d, rows, n in ((512, 1_000_000, 128), (4, 10_000, 100)):
        for family in ("logistic", "linear", "poisson"):
            model, dist, X, y, lat = _problem(family, d, rows, n)
            s = {"w": lat[:, :d], "intercept": lat[:, d]}
            assert U._packed_view(s["w"], s["intercept"], n, d) is not None
            flop = 2 * n * rows * d
            read = rows * d * 4 + rows * 4 + n * (d + 1) * 4
            shape = f"{family} d={d} rows={rows} n={n}"
            t_rows = _time(lambda: U.log_likelihood(model, s, X, y), reps)
            out.append(_line(f"rows form {shape}", t_rows, flop, read + n * rows * 4))
            t_lppd = _time(lambda: U.log_predictive_density(model, s, X, y), reps)
            W, b = lat[:, :d].contiguous(), lat[:, d].contiguous()

            def torch_comp():
                ll = dist(torch.matmul(W, X.T) + b[:, None]).log_prob(y)
                return torch.logsumexp(ll, dim=0) - math.log(n)
            t_comp = _time(torch_comp, max(3, reps // 2))
            out.append(_line(f"lppd form {shape}", t_lppd, flop, read + rows * 4, {"speedup_over_torch": round(t_comp[0] / t_lppd[0], 2)}))
            out.append(_line(f"torch composition {shape}", t_comp, flop, read + rows * 4 + 4 * n * rows * 4))
            got, ref = U.log_predictive_density(model, s, X, y), torch_comp()      # the two compute the same thing
            err = float((got - ref).abs().max())
            print(json.dumps({"case": f"lppd form against the torch composition {shape}", "max_abs_difference": err}), flush=True)
            del X, y, lat, W, b, got, ref
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    L.require_device()
    cases(args.reps)


if __name__ == "__main__":
    main()
