#!/usr/bin/env python3
"""Times of the posterior predictive check's reductions against the compositions they replace (developer tool; the figures of
docs/experiments_ppc.md and DESIGN.md section 4s).  Needs an MI355X: there is no CPU path.

    python tools/time_ppc.py [--repeats 7] [--warmup 2] [--out FILE]

Per family (linear, Poisson, logistic) and shape -- d = 512 + intercept, 10^6 rows, 128 draws; and the examples' shape, d = 4 +
intercept, 10^4 rows, 100 draws --

    fused        ppc.predictive_stats(key, model, samples, X, shift)                        (d3p_predict_stats, no n x rows matrix)
    composition  predictive_samples(key, model, samples, X), then in torch float64 per draw: sum and sum of squares of obs - shift,
                 amin, amax and rows - count_nonzero                                         (what a user does by hand today)
    replicate    ppc.replicate_stats(obs, shift) on the resident matrix                      (d3p_rep_stats)
    torch        the five torch reductions alone on the same resident matrix

Each is timed with device events around one call after `--warmup` calls, the two sides of a pair alternating, and the median, the
minimum and the maximum of `--repeats` calls are reported in milliseconds -- one JSON line per (shape, family), also appended to
`--out`.  The fused and composed results are compared by value before anything is timed (sums within the reordering error of a float64
sum, min / max / zeros equal)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random.debug as jax_random  # noqa: E402
from d3p_amd import ppc  # noqa: E402
from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression  # noqa: E402
from d3p_amd.predictive import predictive_samples  # noqa: E402

SHAPES = {"large": (512, 10 ** 6, 128), "example": (4, 10 ** 4, 100)}


def torch_five(obs, shift):
    e = obs.to(torch.float64) - shift
    return torch.stack([e.sum(1), (e * e).sum(1), obs.amin(1).to(torch.float64), obs.amax(1).to(torch.float64),
                        (obs.shape[1] - torch.count_nonzero(obs, dim=1)).to(torch.float64)])


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


def pair(f, g, warmup, repeats):
    """Median / min / max milliseconds of f and g, alternating."""
    for _ in range(warmup):
        f(), g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(repeats):
        tf.append(timed(f))
        tg.append(timed(g))
    summary = lambda t: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
    return summary(tf), summary(tg)


def problem(family, d, rows, n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(rows, d, generator=g, device="cuda")
    w = torch.randn(n, d, generator=g, device="cuda") / d ** 0.5        # predictors of unit scale
    b = 1.0 + 0.1 * torch.randn(n, generator=g, device="cuda")
    model = {"linear": LinearRegression(d, intercept=True, obs_scale=0.5), "poisson": PoissonRegression(d, intercept=True),
             "logistic": LogisticRegression(d, intercept=True)}[family]
    return model, X, {"w": w, "intercept": b}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    L.require_device()
    key = jax_random.PRNGKey(5)
    for shape, (d, rows, n) in SHAPES.items():
        for family in ("linear", "poisson", "logistic"):
            model, X, samples = problem(family, d, rows, n)
            shift = 1.0
            fused = lambda: ppc.predictive_stats(key, model, samples, X, shift=shift)
            composed = lambda: torch_five(predictive_samples(key, model, samples, X), shift)
            st, ref = fused(), composed()
            got = torch.stack(list(st._five()))
            assert torch.equal(got[2:], ref[2:]), (shape, family, "min / max / zeros differ")
            err = ((got[:2] - ref[:2]).abs() / ref[:2].abs().clamp_min(1.0)).max().item()
            assert err < 1e-7, (shape, family, err)   # (a sanity check of the pairing, not the test: tests/test_gpu_ppc.py)
            del st, ref, got
            t_fused, t_comp = pair(fused, composed, args.warmup, args.repeats)
            obs = predictive_samples(key, model, samples, X)
            t_rep, t_torch = pair(lambda: ppc.replicate_stats(obs, shift), lambda: torch_five(obs, shift), args.warmup, args.repeats)
            line = json.dumps({"shape": shape, "d": d, "rows": rows, "draws": n, "family": family, "repeats": args.repeats,
                               "fused_predictive_stats": t_fused, "composition_samples_then_torch": t_comp,
                               "replicate_stats": t_rep, "torch_reductions": t_torch})
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del obs, X, samples
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
