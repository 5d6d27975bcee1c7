#!/usr/bin/env python3
"""Times d3p_amd.mixture_density's reduced form and rows form with device events after a warm-up (developer tool).

    python tools/time_mixture_density.py [--reps 20]

Shapes: BASELINE config 3's (k = 16, d = 64, 8192 rows, n = 128 draws) and the example's (k = 3, d = 2, 4096 rows, n = 100).  Per shape:
the reduced form (d3p_gmm_loglik_reduce, both outputs in one pass, on latents drawn beforehand), the rows form (d3p_gmm_loglik_rows)
and a torch composition: a loop over the draws of broadcast Normal.log_prob sums, logsumexp, softmax and a running mean.  Per line:
microseconds (median, minimum and maximum over the repetitions); for the two kernels also the terms per second (one term = one
(draw, row, component, dimension)).  Fails without a GPU."""
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
from d3p_amd import mixture as MX  # noqa: E402
from d3p_amd._lib import check, ptr, stream_ptr  # noqa: E402
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
    for k, d, rows, n in ((16, 64, 8192, 128), (3, 2, 4096, 100)):
        g = torch.Generator(device="cuda").manual_seed(0)
        params = {"alpha_log": 0.3 * torch.randn(k, device="cuda", generator=g), "mus_loc": 3 * torch.randn((k, d), device="cuda", generator=g)}
        shape = f"k={k} d={d} rows={rows} n={n}"
        res = MX.posterior_predictive_samples(key, n, model, (k, None, rows, d), guide, params)
        X = res["obs"][0].contiguous()   # held-out points: one draw's outcomes
        latent = torch.cat([res["pis"], res["mus"].reshape(n, -1), res["sigs"].reshape(n, -1)], dim=1).contiguous()
        ld = latent.shape[1]
        ll = torch.empty((n, rows), device="cuda")
        lppd, resp = torch.empty(rows, device="cuda"), torch.empty((rows, k), device="cuda")

        def reduced():
            check(lib.d3p_gmm_loglik_reduce(stream_ptr(), ptr(X), rows, d, ptr(latent), ld, k, n, ptr(lppd), ptr(resp)))

        def rows_form():
            check(lib.d3p_gmm_loglik_rows(stream_ptr(), ptr(X), rows, d, ptr(latent), ld, k, n, ptr(ll)))

        def composition():
            run_lse = torch.full((rows,), -math.inf, device="cuda")
            mean = torch.zeros((rows, k), device="cuda")
            for s in range(n):
                a = torch.distributions.Normal(res["mus"][s], res["sigs"][s]).log_prob(X[:, None, :]).sum(dim=2) + torch.log(res["pis"][s])
                lls = torch.logsumexp(a, dim=1)
                run_lse = torch.logaddexp(run_lse, lls)
                mean += torch.softmax(a, dim=1)
            return run_lse - math.log(n), mean / n

        terms = n * rows * k * d
        t_red = _time(reduced, reps)
        t_rows = _time(rows_form, reps)
        t_comp = _time(composition, max(3, reps // 4))
        ref_lppd, ref_resp = composition()
        agree = {"max_abs_lppd_diff_vs_torch": float((ref_lppd - lppd).abs().max()), "max_abs_resp_diff_vs_torch": float((ref_resp - resp).abs().max())}
        _line(f"d3p_gmm_loglik_reduce {shape}", t_red, dict({"terms_per_s": round(terms / (t_red[0] * 1e-6) / 1e9, 2) * 1e9,
                                                             "torch_over_this": round(t_comp[0] / t_red[0], 2)}, **agree))
        _line(f"d3p_gmm_loglik_rows {shape}", t_rows, {"terms_per_s": round(terms / (t_rows[0] * 1e-6) / 1e9, 2) * 1e9,
                                                       "bytes_written": n * rows * 4})
        _line(f"torch composition {shape}", t_comp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    L.require_device()
    cases(a.reps)


if __name__ == "__main__":
    main()
