#!/usr/bin/env python3
"""Times the WAIC forms of k_loglik and k_gmm_density (d3p_amd.criteria) with device events after a warm-up (developer tool).

    python tools/time_waic.py [--reps 20]

Shapes: tools/time_loglik.py's for the three regression families (10^6 rows, d = 512 + intercept, 128 draws; the example's d = 4,
10^4 rows, 100 draws) and tools/time_mixture_density.py's for the mixture model (k = 16, d = 64, 8192 rows, 128 draws; the
example's k = 3, d = 2, 4096 rows, 100 draws).  Per shape, on latents prepared beforehand (one packed buffer: nothing is copied
before a launch):

  (a) the WAIC entry (d3p_loglik_waic / d3p_gmm_loglik_waic) and the lppd entry of the same shape (d3p_loglik_lppd /
      d3p_gmm_loglik_reduce with lppd alone), ALTERNATING in one loop, so that both see the same state of the machine;
  (b) a torch composition of the same outputs: the rows form (the n x rows matrix is written), torch.logsumexp - log n and
      torch.var over the draws.

Per line: microseconds (median, minimum and maximum over the repetitions); the WAIC line carries waic_over_lppd (ratio of the
medians) and torch_over_this, and the largest differences of its two outputs from the composition's.  Fails without a GPU."""
import argparse
import ctypes as C
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
from d3p_amd import mixture as MX  # noqa: E402
from d3p_amd._lib import check, ptr, stream_ptr  # noqa: E402
from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel  # noqa: E402
from tools.time_loglik import _problem  # noqa: E402


def _event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def _stats(ts):
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def _time_alternating(fns, reps, warmup=3):
    """Every function once per repetition, in turn: [(median, min, max)] in the order given."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(_event_us(fn))
    return [_stats(t) for t in ts]


def _line(name, us, extra=None):
    rec = {"case": name, "us_median": round(us[0], 1), "us_min": round(us[1], 1), "us_max": round(us[2], 1)}
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)


def _report(shape, names, waic_fn, lppd_fn, comp_fn, outs, reps):
    t_waic, t_lppd = _time_alternating([waic_fn, lppd_fn], reps)
    t_comp = _time_alternating([comp_fn], max(3, reps // 4), warmup=1)[0]
    ref_lppd, ref_var = comp_fn()
    waic_fn()
    torch.cuda.synchronize()
    agree = {"max_abs_lppd_diff_vs_torch": float((ref_lppd - outs[0]).abs().max()),
             "max_rel_pwaic_diff_vs_torch": float(((ref_var - outs[1]).abs() / ref_var.abs().clamp_min(1e-30)).max())}
    _line(f"{names[0]} {shape}", t_waic, dict({"waic_over_lppd": round(t_waic[0] / t_lppd[0], 3), "torch_over_this": round(t_comp[0] / t_waic[0], 2)},
                                              **agree))
    _line(f"{names[1]} {shape}", t_lppd)
    _line(f"torch composition (rows form, logsumexp, var) {shape}", t_comp)


def regression_cases(reps):
    lib = L.load()
    for d, rows, n in ((512, 1_000_000, 128), (4, 10_000, 100)):
        for family in ("logistic", "linear", "poisson"):
            model, _, X, y, lat = _problem(family, d, rows, n)
            ms = U._model_struct(model, U._family(model), d)
            lppd, pw, alone = (torch.empty(rows, device="cuda") for _ in range(3))
            s = {"w": lat[:, :d], "intercept": lat[:, d]}

            def waic_form():
                check(lib.d3p_loglik_waic(stream_ptr(), C.byref(ms), ptr(X), ptr(y), rows, ptr(lat), d + 1, 0, d, n, 1, ptr(lppd), ptr(pw)))

            def lppd_form():
                check(lib.d3p_loglik_lppd(stream_ptr(), C.byref(ms), ptr(X), ptr(y), rows, ptr(lat), d + 1, 0, d, n, ptr(alone)))

            def composition():
                ll = U.log_likelihood(model, s, X, y)["obs"]
                return torch.logsumexp(ll, dim=0) - math.log(n), torch.var(ll, dim=0, correction=1)

            _report(f"{family} d={d} rows={rows} n={n}", ("d3p_loglik_waic", "d3p_loglik_lppd"), waic_form, lppd_form, composition, (lppd, pw), reps)
            del X, y, lat, lppd, pw, alone
            torch.cuda.empty_cache()


def mixture_cases(reps):
    lib = L.load()
    key = jr.PRNGKey(0)
    model = GaussianMixtureModel()
    guide = GaussianMixtureGuide(model)
    for k, d, rows, n in ((16, 64, 8192, 128), (3, 2, 4096, 100)):
        g = torch.Generator(device="cuda").manual_seed(0)
        params = {"alpha_log": 0.3 * torch.randn(k, device="cuda", generator=g), "mus_loc": 3 * torch.randn((k, d), device="cuda", generator=g)}
        res = MX.posterior_predictive_samples(key, n, model, (k, None, rows, d), guide, params)
        X = res["obs"][0].contiguous()   # held-out points: one draw's outcomes
        latent = torch.cat([res["pis"], res["mus"].reshape(n, -1), res["sigs"].reshape(n, -1)], dim=1).contiguous()
        ld = latent.shape[1]
        ll = torch.empty((n, rows), device="cuda")
        lppd, pw, alone = (torch.empty(rows, device="cuda") for _ in range(3))

        def waic_form():
            check(lib.d3p_gmm_loglik_waic(stream_ptr(), ptr(X), rows, d, ptr(latent), ld, k, n, 1, ptr(lppd), ptr(pw)))

        def lppd_form():
            check(lib.d3p_gmm_loglik_reduce(stream_ptr(), ptr(X), rows, d, ptr(latent), ld, k, n, ptr(alone), None))

        def composition():
            check(lib.d3p_gmm_loglik_rows(stream_ptr(), ptr(X), rows, d, ptr(latent), ld, k, n, ptr(ll)))
            return torch.logsumexp(ll, dim=0) - math.log(n), torch.var(ll, dim=0, correction=1)

        _report(f"k={k} d={d} rows={rows} n={n}", ("d3p_gmm_loglik_waic", "d3p_gmm_loglik_reduce (lppd alone)"), waic_form, lppd_form, composition,
                (lppd, pw), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    L.require_device()
    regression_cases(a.reps)
    mixture_cases(a.reps)


if __name__ == "__main__":
    main()
