#!/usr/bin/env python3
"""Times the mixture's draw-sums form (d3p_gmm_loglik_draw_sums) and d3p_amd.mixture_diagnostics.guide_diagnostic with device events
after a warm-up (developer tool).

    python tools/time_mixture_diag.py [--reps 10] [--small]

Shapes: BASELINE config 3's k = 16, d = 64 with 128 draws at 8192 rows and at 10^6 rows, and the example's k = 3, d = 2, 2048 rows, 100
draws (--small: without the 10^6 rows).  Per shape, on latents drawn beforehand (one packed buffer, nothing is copied before a launch)
and workspaces allocated once:

  the sums   d3p_gmm_loglik_draw_sums, both of its launches;
  (a)        d3p_gmm_loglik_reduce with lppd only: the same arithmetic per (draw, row), a reduction over the draws instead of the rows;
  (b)        the rows form d3p_gmm_loglik_rows in row slabs of 64 MiB into one reused buffer, each followed by
             ll.sum(1, dtype=torch.float64) added to a running total: the only route there was (the whole matrix is 512 MB at 10^6 rows);
  end to end guide_diagnostic (the draws, the sums, the prior and guide densities, the totals and the Pareto fit).

The sums, (a) and (b) ALTERNATE in one loop, so that all three see the same state of the machine.  Per line: microseconds (median,
minimum and maximum over the repetitions); the sums' line carries the ratios of the medians to (a) and (b), the strips, the terms per
second (one term = one (draw, row, component, dimension)) and the largest relative difference of its sums from (b)'s.  Fails without a
GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random.debug as jr  # noqa: E402
from d3p_amd import mixture as MX  # noqa: E402
from d3p_amd import mixture_diagnostics as MDG  # noqa: E402
from d3p_amd._lib import check, ptr, stream_ptr  # noqa: E402
from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel  # noqa: E402
from tools.time_waic import _line, _time_alternating  # noqa: E402

SLAB_BYTES = 64 << 20


def cases(reps, shapes):
    key = jr.PRNGKey(0)
    model = GaussianMixtureModel()
    guide = GaussianMixtureGuide(model)
    lib = L.load()
    for k, d, rows, n in shapes:
        g = torch.Generator(device="cuda").manual_seed(0)
        params = {"alpha_log": 0.3 * torch.randn(k, device="cuda", generator=g), "mus_loc": 3 * torch.randn((k, d), device="cuda", generator=g)}
        shape = f"k={k} d={d} rows={rows} n={n}"
        z = torch.randint(0, k, (rows,), device="cuda", generator=g)
        X = (params["mus_loc"][z] + torch.randn((rows, d), device="cuda", generator=g)).contiguous()
        draws = MX.posterior_predictive_samples(key, n, model, (k, None, 64, d), guide, params)
        lat = draws["pis"]                      # (the first column of the packed buffer: its data pointer is the buffer's)
        ld = k + 2 * k * d
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        nbytes = lib.d3p_gmm_loglik_draw_sums_workspace(rows, d, k, n)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
        lppd = torch.empty(rows, device="cuda")
        chunk = max(1, min(rows, SLAB_BYTES // (4 * n)))
        slab = torch.empty((n, chunk), device="cuda")
        total = torch.zeros(n, dtype=torch.float64, device="cuda")

        def draw_sums():
            check(lib.d3p_gmm_loglik_draw_sums(stream_ptr(), ptr(X), rows, d, ptr(lat), ld, k, n, ptr(out), ptr(ws), nbytes))

        def reduce_lppd():
            check(lib.d3p_gmm_loglik_reduce(stream_ptr(), ptr(X), rows, d, ptr(lat), ld, k, n, ptr(lppd), None))

        def rows_and_sum():
            total.zero_()
            for lo in range(0, rows, chunk):
                cnt = min(chunk, rows - lo)
                buf = slab.view(-1)[:n * cnt].view(n, cnt)
                check(lib.d3p_gmm_loglik_rows(stream_ptr(), ptr(X[lo:lo + cnt]), cnt, d, ptr(lat), ld, k, n, ptr(buf)))
                total.add_(buf.sum(1, dtype=torch.float64))
            return total

        def end_to_end():
            return MDG.guide_diagnostic(key, n, model, (k, X), guide, params)

        t_sums, t_a, t_b = _time_alternating([draw_sums, reduce_lppd, rows_and_sum], reps)
        t_diag = _time_alternating([end_to_end], reps)[0]
        ref = rows_and_sum().clone()
        draw_sums()
        torch.cuda.synchronize()
        _line(f"d3p_gmm_loglik_draw_sums {shape}", t_sums,
              {"over_reduce_lppd": round(t_sums[0] / t_a[0], 3), "over_rows_and_sum": round(t_sums[0] / t_b[0], 3),
               "strips": nbytes // (8 * n), "gterms_per_s": round(n * rows * k * d / (t_sums[0] * 1e-6) / 1e9, 1),
               "max_rel_diff_vs_rows_and_sum": float(((ref - out).abs() / ref.abs().clamp_min(1e-30)).max())})
        _line(f"(a) d3p_gmm_loglik_reduce, lppd only {shape}", t_a)
        _line(f"(b) d3p_gmm_loglik_rows in {-(-rows // chunk)} slab(s) + float64 row sums {shape}", t_b)
        _line(f"guide_diagnostic end to end {shape}", t_diag)
        del X, ws, lppd, slab
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="without the 10^6-row shape")
    a = ap.parse_args()
    L.require_device()
    shapes = [(16, 64, 8192, 128), (16, 64, 1_000_000, 128), (3, 2, 2048, 100)]
    cases(a.reps, [s for s in shapes if not (a.small and s[2] >= 1_000_000)])


if __name__ == "__main__":
    main()
