#!/usr/bin/env python3
"""Times predictive sampling (d3p_amd.modelling) with device events after a warm-up (developer tool).

    python tools/time_predictive.py [--reps 10]

Cases: the fused logistic path (d3p_predict_logreg + the draws launch) at d = 512, rows = 10^6, n = 128 and at the reference example's
shape (d = 4, rows = 10^4, n = 100); a torch composition of the same logistic work (torch.matmul, sigmoid, then
d3p_amd.random.debug.uniform per draw and a compare); the VAE at n = 10, B = 1 (examples/vae.py:294) and n = 1, B = 4096.  Per case:
microseconds, FLOP/s, the fraction of the 157.3 TFLOP/s fp32 rate and the algorithmic bytes (X read once, latent rows, int32
outcomes written).  Fails without a GPU (no fallback)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random.debug as jr  # noqa: E402
from d3p_amd import modelling as M  # noqa: E402
from d3p_amd.models import AutoDiagonalNormal, LogisticRegression, VAEGuide, VAEModel  # noqa: E402

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


def logreg_cases(reps):
    out = []
    for d, rows, n in ((512, 1_000_000, 128), (4, 10_000, 100)):
        model = LogisticRegression(d, intercept=True)
        guide = AutoDiagonalNormal(model)
        params = {"auto_loc": 0.1 * torch.randn(d + 1, device="cuda"), "auto_scale": torch.full((d + 1,), 0.1, device="cuda")}
        X = torch.randn((rows, d), device="cuda")
        key = jr.PRNGKey(0)
        flop = 2 * n * rows * d
        nbytes = rows * d * 4 + n * (d + 1) * 4 + n * rows * 4
        fused = _time(lambda: M.sample_multi_posterior_predictive(key, n, model, (X,), guide, (X,), params), reps)
        out.append(_line(f"logreg fused d={d} rows={rows} n={n}", fused, flop, nbytes))
        res = M.sample_multi_posterior_predictive(key, n, model, (X,), guide, (X,), params)
        W, b = res["w"].contiguous(), res["intercept"].contiguous()
        okeys = jr.split(key, n)   # (stand-in keys: the composition's cost, not its stream)

        def torch_comp():
            p = torch.sigmoid(torch.matmul(W, X.T) + b[:, None])
            obs = torch.empty((n, rows), dtype=torch.int32, device="cuda")
            for i in range(n):
                obs[i] = (jr.uniform(okeys[i], (rows,)) < p[i]).to(torch.int32)
            return obs
        comp = _time(torch_comp, max(3, reps // 2))
        out.append(_line(f"logreg torch composition d={d} rows={rows} n={n}", comp, flop,
                         nbytes + 3 * n * rows * 4, {"fused_speedup": round(comp[0] / fused[0], 2)}))
    return out


def vae_cases(reps):
    out = []
    D, H, Z = 784, 400, 50
    from d3p_amd._lib import VaeModel
    shapes, n_dec = M._vae_leaf_shapes(VaeModel(D, H, Z, 1.0, 1.0, 0))
    flat = 0.05 * torch.randn(sum(int(np.prod(s)) for s in shapes), device="cuda")
    model = VAEModel(Z, H)
    for n, B in ((10, 1), (1, 4096)):
        X = (torch.rand((B, D), device="cuda") < 0.2).float()
        key = jr.PRNGKey(0)
        flop = 2 * B * (D * H + 2 * H * Z) + 2 * n * B * (Z * H + H * D)
        nbytes = B * D * 4 + flat.numel() * 4 + n * B * (Z + D) * 4
        t = _time(lambda: M.sample_multi_posterior_predictive(key, n, model, (B, Z, H, D), VAEGuide(model), (X, Z, H), flat), reps)
        out.append(_line(f"vae 784-400-50 n={n} B={B}", t, flop, nbytes))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    L.require_device()
    logreg_cases(args.reps)
    vae_cases(args.reps)


if __name__ == "__main__":
    main()
