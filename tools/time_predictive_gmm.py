#!/usr/bin/env python3
"""Times d3p_amd.mixture.posterior_predictive_samples and assign with device events after a warm-up (developer tool).

    python tools/time_predictive_gmm.py [--reps 20]

Shapes: BASELINE config 3's (k = 16, d = 64, 8192 rows, n = 128 draws) and the example's (k = 3, d = 2, 4096 rows, n = 1).  Per shape:
the whole call (latent draws + outcomes), the outcome kernel alone (d3p_predict_gmm_obs on latents drawn beforehand), a torch
composition that loops GaussianMixture.sample_with_intermediates over the draws, assign, and cdist / argmin on the same points.
Per line: microseconds (median, minimum and maximum over the repetitions); for the outcome kernel also the threefry calls per second
(one call per two outcomes, plus one per row for the component) and the bytes written over the time.  Fails without a GPU."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random.debug as jr  # noqa: E402
from d3p_amd import mixture as MX  # noqa: E402
from d3p_amd._lib import check, ptr, stream_ptr  # noqa: E402
from d3p_amd.gmm import GaussianMixture  # noqa: E402
from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel  # noqa: E402


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


def _line(name, us, extra=None):
    rec = {"case": name, "us_median": round(us[0], 1), "us_min": round(us[1], 1), "us_max": round(us[2], 1)}
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)


def cases(reps):
    key = jr.PRNGKey(0)
    model = GaussianMixtureModel()
    guide = GaussianMixtureGuide(model)
    lib = L.load()
    for k, d, rows, n in ((16, 64, 8192, 128), (3, 2, 4096, 1)):
        g = torch.Generator(device="cuda").manual_seed(0)
        params = {"alpha_log": 0.3 * torch.randn(k, device="cuda", generator=g), "mus_loc": 3 * torch.randn((k, d), device="cuda", generator=g)}
        shape = f"k={k} d={d} rows={rows} n={n}"
        args = (k, None, rows, d)
        res = MX.posterior_predictive_samples(key, n, model, args, guide, params)
        latent = torch.cat([res["pis"], res["mus"].reshape(n, -1), res["sigs"].reshape(n, -1)], dim=1).contiguous()
        obs_keys = jr.split(key, n).contiguous()
        obs = torch.empty((n, rows, d), device="cuda")

        def kernel_only():
            check(lib.d3p_predict_gmm_obs(stream_ptr(), ptr(latent), latent.shape[1], k, d, rows, n, ptr(obs_keys), ptr(obs), None))

        def composition():
            out = []
            for s in range(n):
                gm = GaussianMixture(res["mus"][s], res["sigs"][s], res["pis"][s])
                out.append(gm.sample_with_intermediates(obs_keys[s], (rows,))[0])
            return torch.stack(out)

        t_all = _time(lambda: MX.posterior_predictive_samples(key, n, model, args, guide, params), reps)
        t_obs = _time(kernel_only, reps)
        t_comp = _time(composition, max(3, reps // 4))
        calls = n * ((rows * d + 1) // 2 + rows)
        nbytes = n * rows * d * 4
        _line(f"posterior_predictive_samples {shape}", t_all, {"speedup_over_torch": round(t_comp[0] / t_all[0], 2)})
        _line(f"d3p_predict_gmm_obs alone {shape}", t_obs, {"threefry_calls_per_s": round(calls / (t_obs[0] * 1e-6) / 1e9, 2) * 1e9,
                                                           "bytes_written": nbytes, "TB_per_s": round(nbytes / (t_obs[0] * 1e-6) / 1e12, 3)})
        _line(f"torch composition {shape}", t_comp)
        X = res["obs"][0]
        mus, sigs, pis = res["mus"][0], torch.ones((k, d), device="cuda"), res["pis"][0]
        t_assign = _time(lambda: MX.assign(X, mus, sigs, pis), reps)
        t_cdist = _time(lambda: torch.cdist(X, mus).argmin(dim=1), reps)
        _line(f"assign {shape}", t_assign, {"over_cdist_argmin": round(t_assign[0] / t_cdist[0], 2)})
        _line(f"cdist / argmin {shape}", t_cdist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    L.require_device()
    cases(a.reps)


if __name__ == "__main__":
    main()
