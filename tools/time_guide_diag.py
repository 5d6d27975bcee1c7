#!/usr/bin/env python3
"""Times the draw-sums form (d3p_loglik_draw_sums) and d3p_amd.diagnostics.guide_diagnostic with device events after a warm-up
(developer tool).

    python tools/time_guide_diag.py [--reps 20] [--small]

Shapes: tools/time_loglik.py's -- the three regression families at 10^6 rows, d = 512 + intercept, 128 draws and at the examples'
d = 4, 10^4 rows, 100 draws (--small: the examples' shape only).  Per shape, on latents prepared beforehand (one packed buffer:
nothing is copied before a launch):

  (a) d3p_loglik_draw_sums alone (both of its launches, the workspace allocated once) and the lppd form d3p_loglik_lppd at the same
      shape -- the parent's nearest kernel: the same product, a reduction over the draws instead of the rows -- ALTERNATING in one loop,
      so that both see the same state of the machine;
  (b) guide_diagnostic end to end (the draws, the sums, the prior and guide densities, the totals and the Pareto fit);
  (c) a torch composition of (a): matmul, the family's log_prob, .double().sum(1) (the n x rows matrix is written).

Per line: microseconds (median, minimum and maximum over the repetitions); line (a) carries draw_sums_over_lppd (ratio of the
medians), torch_over_this, achieved FLOP/s and bytes/s of the product (2 n rows d operations; X, y and the latents read once) and
the largest relative difference of its sums from the composition's.  Fails without a GPU."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random.debug as jr  # noqa: E402
from d3p_amd import diagnostics as DG  # noqa: E402
from d3p_amd import infer_util as U  # noqa: E402
from d3p_amd._lib import check, ptr, stream_ptr  # noqa: E402
from d3p_amd.models import AutoDiagonalNormal  # noqa: E402
from tools.time_loglik import _problem  # noqa: E402
from tools.time_waic import _line, _time_alternating  # noqa: E402


def cases(reps, shapes):
    lib = L.load()
    key = jr.PRNGKey(0)
    for d, rows, n in shapes:
        for family in ("logistic", "linear", "poisson"):
            model, dist, X, y, lat = _problem(family, d, rows, n)
            ms = U._model_struct(model, U._family(model), d)
            shape = f"{family} d={d} rows={rows} n={n}"
            out = torch.empty(n, dtype=torch.float64, device="cuda")
            nbytes = lib.d3p_loglik_draw_sums_workspace(rows, n)
            ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
            alone = torch.empty(rows, device="cuda")

            def draw_sums():
                check(lib.d3p_loglik_draw_sums(stream_ptr(), C.byref(ms), ptr(X), ptr(y), rows, ptr(lat), d + 1, 0, d, n, ptr(out), ptr(ws), nbytes))

            def lppd_form():
                check(lib.d3p_loglik_lppd(stream_ptr(), C.byref(ms), ptr(X), ptr(y), rows, ptr(lat), d + 1, 0, d, n, ptr(alone)))

            def composition():
                t = lat[:, :d] @ X.T + lat[:, d:d + 1]
                return dist(t).log_prob(y).double().sum(1)

            guide = AutoDiagonalNormal(model)
            params = {"auto_loc": lat[0].clone(), "auto_scale": torch.full((d + 1,), 0.01, device="cuda")}

            def end_to_end():
                return DG.guide_diagnostic(key, n, model, (X, y), guide, params)

            t_sums, t_lppd = _time_alternating([draw_sums, lppd_form], reps)
            t_diag = _time_alternating([end_to_end], reps)[0]
            t_comp = _time_alternating([composition], max(3, reps // 4), warmup=1)[0]
            ref = composition()
            draw_sums()
            torch.cuda.synchronize()
            s = t_sums[0] * 1e-6
            _line(f"d3p_loglik_draw_sums {shape}", t_sums,
                  {"draw_sums_over_lppd": round(t_sums[0] / t_lppd[0], 3), "torch_over_this": round(t_comp[0] / t_sums[0], 2),
                   "strips": nbytes // (8 * n), "tflops": round(2.0 * n * rows * d / s / 1e12, 2),
                   "gbytes_per_s": round((rows * d * 4 + rows * 4 + n * (d + 1) * 4) / s / 1e9, 1),
                   "max_rel_diff_vs_torch": float(((ref - out).abs() / ref.abs().clamp_min(1e-30)).max())})
            _line(f"d3p_loglik_lppd {shape}", t_lppd)
            _line(f"guide_diagnostic end to end {shape}", t_diag)
            _line(f"torch composition (matmul, log_prob, double sum) {shape}", t_comp)
            del X, y, lat, ws, alone
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="the examples' shape only")
    a = ap.parse_args()
    L.require_device()
    cases(a.reps, ((4, 10_000, 100),) if a.small else ((512, 1_000_000, 128), (4, 10_000, 100)))


if __name__ == "__main__":
    main()
