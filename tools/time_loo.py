#!/usr/bin/env python3
"""Times PSIS-LOO (d3p_amd.criteria.loo, d3p_psis_loo) with device events after a warm-up (developer tool).

    python tools/time_loo.py [--reps 20] [--small]

Shapes: tools/time_waic.py's -- the three regression families at 10^6 rows, d = 512 + intercept, 128 draws and at the example's
d = 4, 10^4 rows, 100 draws; the mixture model at k = 16, d = 64, 8192 rows, 128 draws and at the example's k = 3, d = 2, 4096 rows,
100 draws (--small: the examples' shapes only).  Per shape, on latents prepared beforehand (one packed buffer: nothing is copied
before a launch):

  (a) criteria.loo and criteria.waic on the same samples, ALTERNATING in one loop, so that both see the same state of the machine
      (loo at its default slab size: the rows entry and d3p_psis_loo per slab of 64 MiB);
  (b) d3p_psis_loo alone on one resident slab of the matrix (the default slab's rows, or all of them where they are fewer);
  (c) the floor of any torch composition: the rows entry for that slab followed by torch.topk(M + 1) over the draws -- the order
      statistic alone, none of the fit.

Per line: microseconds (median, minimum and maximum over the repetitions); line (a) carries loo_over_waic (ratio of the medians),
line (b) rows_per_s and the bytes of the slab.  Fails without a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random.debug as jr  # noqa: E402
from d3p_amd import criteria as CR  # noqa: E402
from d3p_amd import infer_util as U  # noqa: E402
from d3p_amd import mixture as MX  # noqa: E402
from d3p_amd._lib import check, ptr, stream_ptr  # noqa: E402
from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel  # noqa: E402
from tools.time_loglik import _problem  # noqa: E402
from tools.time_waic import _line, _time_alternating  # noqa: E402

SLAB = 64 << 20


def _tail_len(n):
    import math
    return int(math.ceil(min(n / 5.0, 3.0 * math.sqrt(n))))


def _report(shape, n, rows, loo_fn, waic_fn, fill_slab, reps):
    """fill_slab(count, buf) launches the rows entry for the first `count` rows into buf (n x count)."""
    lib = L.load()
    t_loo, t_waic = _time_alternating([loo_fn, waic_fn], reps)
    _line(f"criteria.loo {shape}", t_loo, {"loo_over_waic": round(t_loo[0] / t_waic[0], 2)})
    _line(f"criteria.waic {shape}", t_waic)
    count = min(U._loo_chunk(n, SLAB), rows)
    buf = torch.empty((n, count), device="cuda")
    elpd, lppd, khat = (torch.empty(count, device="cuda") for _ in range(3))
    fill_slab(count, buf)

    def psis_alone():
        check(lib.d3p_psis_loo(stream_ptr(), ptr(buf), count, n, count, ptr(elpd), ptr(lppd), ptr(khat)))

    def rows_and_topk():
        fill_slab(count, buf)
        return torch.topk(buf, min(_tail_len(n) + 1, n), dim=0, largest=False, sorted=False)

    t_psis, t_floor = _time_alternating([psis_alone, rows_and_topk], reps)
    _line(f"d3p_psis_loo alone, {count} resident rows {shape}", t_psis,
          {"rows_per_s": round(count / (t_psis[0] * 1e-6)), "slab_bytes": 4 * n * count, "high_k_rows": int((~(khat <= CR._k_threshold(n))).sum())})
    _line(f"rows entry + torch.topk(M + 1 = {_tail_len(n) + 1}), the same slab {shape}", t_floor)


def regression_cases(reps, shapes):
    lib = L.load()
    for d, rows, n in shapes:
        for family in ("logistic", "linear", "poisson"):
            model, _, X, y, lat = _problem(family, d, rows, n)
            ms = U._model_struct(model, U._family(model), d)
            s = {"w": lat[:, :d], "intercept": lat[:, d]}

            def fill_slab(count, buf):
                check(lib.d3p_loglik_rows(stream_ptr(), C.byref(ms), ptr(X), ptr(y), count, ptr(lat), d + 1, 0, d, n, ptr(buf)))

            _report(f"{family} d={d} rows={rows} n={n}", n, rows, lambda: CR.loo(model, s, X, y), lambda: CR.waic(model, s, X, y), fill_slab, reps)
            del X, y, lat
            torch.cuda.empty_cache()


def mixture_cases(reps, shapes):
    lib = L.load()
    key = jr.PRNGKey(0)
    model = GaussianMixtureModel()
    guide = GaussianMixtureGuide(model)
    for k, d, rows, n in shapes:
        g = torch.Generator(device="cuda").manual_seed(0)
        params = {"alpha_log": 0.3 * torch.randn(k, device="cuda", generator=g), "mus_loc": 3 * torch.randn((k, d), device="cuda", generator=g)}
        res = MX.posterior_predictive_samples(key, n, model, (k, None, rows, d), guide, params)
        X = res["obs"][0].contiguous()   # held-out points: one draw's outcomes
        s = {name: res[name] for name in ("pis", "mus", "sigs")}
        latent = torch.cat([res["pis"], res["mus"].reshape(n, -1), res["sigs"].reshape(n, -1)], dim=1).contiguous()
        ld = latent.shape[1]

        def fill_slab(count, buf):
            check(lib.d3p_gmm_loglik_rows(stream_ptr(), ptr(X), count, d, ptr(latent), ld, k, n, ptr(buf)))

        _report(f"mixture k={k} d={d} rows={rows} n={n}", n, rows, lambda: CR.loo(model, s, X), lambda: CR.waic(model, s, X), fill_slab, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="the examples' shapes only")
    a = ap.parse_args()
    L.require_device()
    regression_cases(a.reps, ((4, 10_000, 100),) if a.small else ((512, 1_000_000, 128), (4, 10_000, 100)))
    mixture_cases(a.reps, ((3, 2, 4096, 100),) if a.small else ((16, 64, 8192, 128), (3, 2, 4096, 100)))


if __name__ == "__main__":
    main()
