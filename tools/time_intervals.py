#!/usr/bin/env python3
"""Times the credible and predictive intervals (d3p_amd.intervals, d3p_col_quantiles, d3p_predict_mean_rows) with device events after
a warm-up (developer tool).

    python tools/time_intervals.py [--reps 20] [--small]

  (a) d3p_col_quantiles alone on one resident 64 MiB slab of random normal values, at the probabilities (0.05, 0.5, 0.95): 128 draws
      (the staged form: the keys in LDS) and 1024 draws (the streamed form: every pass reads memory), each ALTERNATING with the torch
      composition on the same slab -- torch.sort(dim=0), two gathers and a lerp per probability (torch.quantile refuses inputs of
      this size);
  (b) per family at d = 512 + intercept, 10^6 rows, 128 draws and at the examples' d = 4, 10^4 rows, 100 draws (--small: the latter
      only), on latents prepared beforehand (one packed buffer): credible_interval and criteria.waic on the same samples, alternating;
      one slab of the pair d3p_predict_mean_rows + d3p_col_quantiles against the torch composition on that slab (matmul, the link,
      sort, gathers, lerp); and, linear and Poisson, predictive_interval against predictive_samples alone (the matrix it reduces; its
      slab_bytes is set to the matrix's size, which at 10^6 rows x 128 draws is 512 MB).

Per line: microseconds (median, minimum and maximum over the repetitions) and the ratios of the medians.  Fails without a GPU."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random.debug as jr  # noqa: E402
from d3p_amd import criteria as CR  # noqa: E402
from d3p_amd import infer_util as U  # noqa: E402
from d3p_amd import intervals as IV  # noqa: E402
from d3p_amd import predictive as PS  # noqa: E402
from d3p_amd._lib import check, ptr, stream_ptr  # noqa: E402
from tools.time_loglik import _problem  # noqa: E402
from tools.time_waic import _line, _time_alternating  # noqa: E402

SLAB = 64 << 20
PROBS = (0.05, 0.5, 0.95)


def _torch_quantiles(m, pos):
    """The composition: one sort over the draws, then per probability two gathers and numpy's lerp."""
    s = torch.sort(m, dim=0).values
    n = m.shape[0]
    out = []
    for lo, g in pos:
        a, b = s[lo], s[min(lo + 1, n - 1)]
        d = b - a
        out.append(a + d * g if g < 0.5 else b - d * (1.0 - g))
    return torch.stack(out)


RULE = IV._equal_tailed(PROBS)


def _quantiles_into(buf, n, count, args, out):
    RULE.reduce(buf, torch.float32, count, n, count, args, out, count)


def kernel_alone(reps):
    lib = L.load()
    staged_max = int(lib.d3p_col_quantiles_staged_max())
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in (128, 1024):
        count = U._loo_chunk(n, SLAB)
        buf = torch.randn((n, count), device="cuda", generator=g)
        out = torch.empty((len(PROBS), count), device="cuda")
        pos, args = IV.positions(PROBS, n), RULE.args(n)
        t_k, t_t = _time_alternating([lambda: _quantiles_into(buf, n, count, args, out), lambda: _torch_quantiles(buf, pos)], reps)
        same = bool(torch.equal(out, _torch_quantiles(buf.double(), pos).float()))
        form = "staged" if n <= staged_max else "streamed"
        _line(f"d3p_col_quantiles alone ({form}), n={n} cols={count} Q=3", t_k,
              {"cols_per_s": round(count / (t_k[0] * 1e-6)), "slab_bytes": 4 * n * count, "torch_over_this": round(t_t[0] / t_k[0], 2),
               "equals_float64_torch": same})
        _line(f"torch sort + gathers + lerp, the same slab n={n} cols={count}", t_t)
        del buf
        torch.cuda.empty_cache()


def _link(family, t):
    return torch.sigmoid(t) if family == "logistic" else t if family == "linear" else torch.exp(t)


def regression_cases(reps, shapes):
    lib = L.load()
    key = jr.PRNGKey(0)
    for d, rows, n in shapes:
        for family in ("logistic", "linear", "poisson"):
            model, _, X, y, lat = _problem(family, d, rows, n)
            ms = U._model_struct(model, U._family(model), d)
            s = {"w": lat[:, :d], "intercept": lat[:, d]}
            shape = f"{family} d={d} rows={rows} n={n}"
            pos, args = IV.positions(PROBS, n), RULE.args(n)
            t_ci, t_waic = _time_alternating([lambda: IV.credible_interval(model, s, X, probs=PROBS), lambda: CR.waic(model, s, X, y)], reps)
            _line(f"intervals.credible_interval {shape}", t_ci, {"over_waic": round(t_ci[0] / t_waic[0], 2)})
            _line(f"criteria.waic {shape}", t_waic)
            count = min(U._loo_chunk(n, SLAB), rows)
            buf = torch.empty((n, count), device="cuda")
            out = torch.empty((len(PROBS), count), device="cuda")
            W, b = lat[:, :d].contiguous(), lat[:, d].contiguous()

            def pair():
                check(lib.d3p_predict_mean_rows(stream_ptr(), C.byref(ms), ptr(X), count, ptr(lat), d + 1, 0, d, n, ptr(buf), count))
                _quantiles_into(buf, n, count, args, out)

            def mean_rows_only():
                check(lib.d3p_predict_mean_rows(stream_ptr(), C.byref(ms), ptr(X), count, ptr(lat), d + 1, 0, d, n, ptr(buf), count))

            def composition():
                return _torch_quantiles(_link(family, torch.matmul(W, X[:count].T) + b[:, None]), pos)

            t_pair, t_rows, t_comp = _time_alternating([pair, mean_rows_only, composition], reps)
            _line(f"d3p_predict_mean_rows + d3p_col_quantiles, one slab of {count} rows {shape}", t_pair,
                  {"torch_over_this": round(t_comp[0] / t_pair[0], 2), "slab_bytes": 4 * n * count})
            _line(f"d3p_predict_mean_rows alone, the same slab {shape}", t_rows)
            _line(f"torch matmul + link + sort + gathers + lerp, the same slab {shape}", t_comp)
            del buf, out
            if family != "logistic":
                whole = 4 * n * rows
                t_pi, t_ps = _time_alternating([lambda: IV.predictive_interval(key, model, s, X, probs=PROBS, slab_bytes=whole),
                                                lambda: PS.predictive_samples(key, model, s, X)], max(3, reps // 2))
                _line(f"intervals.predictive_interval {shape}", t_pi, {"over_predictive_samples": round(t_pi[0] / t_ps[0], 2), "matrix_bytes": whole})
                _line(f"predictive.predictive_samples {shape}", t_ps)
            del X, y, lat, W, b
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="the examples' shape only")
    a = ap.parse_args()
    L.require_device()
    kernel_alone(a.reps)
    regression_cases(a.reps, ((4, 10_000, 100),) if a.small else ((512, 1_000_000, 128), (4, 10_000, 100)))


if __name__ == "__main__":
    main()
