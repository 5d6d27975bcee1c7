#!/usr/bin/env python3
"""Times of the realized-discrepancy reduction against the composition it replaces (developer tool; the figures of
docs/experiments_discrepancy.md and DESIGN.md section 4t).  Needs an MI355X: there is no CPU path.

    python tools/time_discrepancy.py [--repeats 7] [--warmup 2] [--out FILE]

Per family (linear, Poisson, logistic) and shape -- d = 512 + intercept, 10^6 rows, 128 draws; and the examples' shape, d = 4 +
intercept, 10^4 rows, 100 draws --

    fused        discrepancy.posterior_predictive_discrepancy(key, n, model, (X, y), guide, params, shift)
                                                             (d3p_predict_discrepancy: neither n x rows matrix is written)
    composition  posterior_predictive_samples(key, n, model, (X,), guide, params), d3p_predict_mean_rows of its latents over the whole
                 table, then in torch float64 per draw the six sums                          (what a user does by hand without the module)
    stats        ppc.posterior_predictive_stats(key, n, model, (X,), guide, params, shift)   (the same tile and outcome rule, a lighter epilogue)

Each is timed with device events around one call after `--warmup` calls, fused and composition alternating, then fused and stats
alternating, and the median, the minimum and the maximum of `--repeats` calls are reported in milliseconds -- one JSON line per (shape,
family), also appended to `--out`.  The fused and composed sums are compared before anything is timed (within the reordering error of a
float64 sum; the test of the values is tests/test_gpu_discrepancy.py)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random.debug as jax_random  # noqa: E402
from d3p_amd import discrepancy, ppc  # noqa: E402
from d3p_amd.infer_util import _model_struct  # noqa: E402
from d3p_amd.models import AutoDiagonalNormal, LinearRegression, LogisticRegression, PoissonRegression  # noqa: E402
from d3p_amd.predictive import _family, posterior_predictive_samples  # noqa: E402

SHAPES = {"large": (512, 10 ** 6, 128), "example": (4, 10 ** 4, 100)}
SIGMA = 0.5


def mean_rows(model, X, w, b):
    """d3p_predict_mean_rows over the whole table: (n, rows) float32."""
    n, d = w.shape
    lat = torch.cat([w, b.reshape(n, 1)], dim=1).contiguous()
    mu = torch.empty((n, X.shape[0]), dtype=torch.float32, device=X.device)
    ms = _model_struct(model, _family(model), d)
    L.check(L.load().d3p_predict_mean_rows(L.stream_ptr(), C.byref(ms), L.ptr(X), X.shape[0], L.ptr(lat), d + 1, 0, d, n, L.ptr(mu), X.shape[0]))
    return mu


def torch_six(family, mu, obs, y, shift):
    M = mu.to(torch.float64)
    V = torch.full_like(M, SIGMA * SIGMA) if family == "linear" else (M if family == "poisson" else M * (1.0 - M))
    ey = y.to(torch.float64)[None, :] - M
    ev = obs.to(torch.float64) - M
    zero = torch.zeros((), dtype=torch.float64, device=M.device)
    m = M - shift
    return torch.stack([torch.where(ey == 0, zero, ey * ey / V).sum(1), torch.where(ev == 0, zero, ev * ev / V).sum(1), m.sum(1), (m * m).sum(1),
                        ey.sum(1), (ey * ey).sum(1)])


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


def problem(family, d, rows, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(rows, d, generator=g, device="cuda")
    loc = torch.cat([torch.randn(d, generator=g, device="cuda") / d ** 0.5, torch.ones(1, device="cuda")])   # predictors of unit scale
    t = X @ loc[:d] + loc[d]
    if family == "linear":
        model = LinearRegression(d, intercept=True, obs_scale=SIGMA)
        y = t + SIGMA * torch.randn(rows, generator=g, device="cuda")
    elif family == "poisson":
        model = PoissonRegression(d, intercept=True)
        y = torch.poisson(torch.exp(t), generator=g)
    else:
        model = LogisticRegression(d, intercept=True)
        y = (torch.rand(rows, generator=g, device="cuda") < torch.sigmoid(t)).to(torch.float32)
    params = {"auto_loc": loc.contiguous(), "auto_scale": torch.full((d + 1,), 0.1 / d ** 0.5, device="cuda")}
    return model, AutoDiagonalNormal(model), params, X, y.to(torch.float32).contiguous()


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
            model, guide, params, X, y = problem(family, d, rows)
            shift = float(y.mean())
            fused = lambda: discrepancy.posterior_predictive_discrepancy(key, n, model, (X, y), guide, params, shift=shift)[1]

            def composed():
                res = posterior_predictive_samples(key, n, model, (X,), guide, params)
                return torch_six(family, mean_rows(model, X, res["w"], res["intercept"]), res["obs"], y, shift)

            stats = lambda: ppc.posterior_predictive_stats(key, n, model, (X,), guide, params, shift=shift)[1]
            got, ref = torch.stack(list(fused()._six())), composed()
            err = ((got - ref).abs() / ref.abs().clamp_min(1.0)).max().item()
            assert err < 1e-7, (shape, family, err)   # (a sanity check of the pairing, not the test: tests/test_gpu_discrepancy.py)
            del got, ref
            t_fused, t_comp = pair(fused, composed, args.warmup, args.repeats)
            t_fused2, t_stats = pair(fused, stats, args.warmup, args.repeats)
            line = json.dumps({"shape": shape, "d": d, "rows": rows, "draws": n, "family": family, "repeats": args.repeats,
                               "fused_discrepancy": t_fused, "composition_samples_mean_rows_torch": t_comp,
                               "fused_discrepancy_beside_stats": t_fused2, "fused_predictive_stats": t_stats})
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del X, y
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
