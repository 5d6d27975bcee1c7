#!/usr/bin/env python3
"""Times of the classification metrics against what they replace (developer tool; the figures of docs/experiments_classification.md and
DESIGN.md section 4u).  Needs an MI355X: there is no CPU path.

    python tools/time_classification.py [--repeats 21] [--warmup 3] [--out FILE]

Per shape -- d = 512 + intercept, 10^6 rows, 128 draws; and the example's shape, d = 4 + intercept, 10^4 rows, 100 draws --

    fused        classification.posterior_predictive_confusion(key, n, model, (X, y), guide, params, thresholds=(0.5,))
                                                             (d3p_predict_confusion: neither n x rows matrix is written)
    composition  posterior_predictive_samples(key, n, model, (X,), guide, params), d3p_predict_mean_rows of its latents over the whole
                 table, then in torch the comparisons with y and the sums per draw  (what a user does by hand without the module)
    discrepancy  discrepancy.posterior_predictive_discrepancy(key, n, model, (X, y), guide, params, shift)
                                                             (the same tile and outcome rule with six float64 sums per draw)

and per score count -- 10^6 and 10^7 --

    curve        classification.binary_curve(p, y, bins=10)  (histogram, reliability table, pair counts, KS numerator; one read-back)
    sort         torch.sort(p, descending=True), the labels gathered, cumulative sums of both classes and the pair count of the exact
                 AUC from them (ties ignored: the cheapest thing a sort-based AUC can be)

Each is timed with device events around one call after `--warmup` calls, the entry and its baseline alternating within this process, and
the median, the minimum and the maximum of `--repeats` calls are reported in milliseconds -- one JSON line per case, also appended to
`--out`.  The fused and composed counts are compared by value before anything is timed (the test of the values is
tests/test_gpu_classification.py)."""
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
from d3p_amd import classification, discrepancy  # noqa: E402
from d3p_amd.infer_util import _model_struct  # noqa: E402
from d3p_amd.models import AutoDiagonalNormal, LogisticRegression  # noqa: E402
from d3p_amd.predictive import _family, posterior_predictive_samples  # noqa: E402

SHAPES = {"large": (512, 10 ** 6, 128), "example": (4, 10 ** 4, 100)}
SCORES = (10 ** 6, 10 ** 7)


def mean_rows(model, X, w, b):
    """d3p_predict_mean_rows over the whole table: (n, rows) float32."""
    n, d = w.shape
    lat = torch.cat([w, b.reshape(n, 1)], dim=1).contiguous()
    mu = torch.empty((n, X.shape[0]), dtype=torch.float32, device=X.device)
    ms = _model_struct(model, _family(model), d)
    L.check(L.load().d3p_predict_mean_rows(L.stream_ptr(), C.byref(ms), L.ptr(X), X.shape[0], L.ptr(lat), d + 1, 0, d, n, L.ptr(mu), X.shape[0]))
    return mu


def torch_counts(mu, obs, y, tau):
    """(agree, tp, fp) per draw from the stored matrices."""
    yi = y.to(torch.int32)
    ge = mu >= tau
    return (obs == yi[None, :]).sum(1), (ge & (yi[None, :] == 1)).sum(1), (ge & (yi[None, :] == 0)).sum(1)


def sort_auc(p, y):
    """(cumulative positives, cumulative negatives, concordant pairs) by a descending sort: the ROC points and the AUC's numerator."""
    order = torch.sort(p, descending=True).indices
    pos = y[order].to(torch.int64)
    cp, cn = torch.cumsum(pos, 0), torch.cumsum(1 - pos, 0)
    return cp, cn, (cp * (1 - pos)).sum()


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


def problem(d, rows, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(rows, d, generator=g, device="cuda")
    loc = torch.cat([torch.randn(d, generator=g, device="cuda") / d ** 0.5, torch.ones(1, device="cuda")])   # predictors of unit scale
    y = (torch.rand(rows, generator=g, device="cuda") < torch.sigmoid(X @ loc[:d] + loc[d])).to(torch.float32)
    model = LogisticRegression(d, intercept=True)
    params = {"auto_loc": loc.contiguous(), "auto_scale": torch.full((d + 1,), 0.1 / d ** 0.5, device="cuda")}
    return model, AutoDiagonalNormal(model), params, X, y.contiguous()


def emit(line, out):
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    L.require_device()
    key = jax_random.PRNGKey(5)
    for shape, (d, rows, n) in SHAPES.items():
        model, guide, params, X, y = problem(d, rows)
        shift = float(y.mean())
        fused = lambda: classification.posterior_predictive_confusion(key, n, model, (X, y), guide, params, thresholds=(0.5,))[1]

        def composed():
            res = posterior_predictive_samples(key, n, model, (X,), guide, params)
            return torch_counts(mean_rows(model, X, res["w"], res["intercept"]), res["obs"], y, 0.5)

        disc = lambda: discrepancy.posterior_predictive_discrepancy(key, n, model, (X, y), guide, params, shift=shift)[1]
        got, ref = fused(), composed()
        assert torch.equal(got.agree, ref[0]) and torch.equal(got.tp[:, 0], ref[1]) and torch.equal(got.fp[:, 0], ref[2]), shape
        del got, ref
        t_fused, t_comp = pair(fused, composed, args.warmup, args.repeats)
        t_fused2, t_disc = pair(fused, disc, args.warmup, args.repeats)
        emit(json.dumps({"case": "confusion", "shape": shape, "d": d, "rows": rows, "draws": n, "repeats": args.repeats,
                         "fused_confusion": t_fused, "composition_samples_mean_rows_torch": t_comp,
                         "fused_confusion_beside_discrepancy": t_fused2, "fused_discrepancy": t_disc}), args.out)
        del X, y
        torch.cuda.empty_cache()
    g = torch.Generator(device="cuda").manual_seed(1)
    for rows in SCORES:
        for scale in (1.0, 8.0):                                      # (8: a sharp classifier, scores piled up at both ends)
            p = torch.sigmoid(torch.randn(rows, generator=g, device="cuda") * scale)
            y = (torch.rand(rows, generator=g, device="cuda") < p).to(torch.int32)
            curve = lambda: classification.binary_curve(p, y, bins=10)
            srt = lambda: sort_auc(p, y)
            c = curve()
            exact = float(srt()[2]) / (float(c.n_pos) * float(c.n_neg))
            assert c.auc_lo - 1e-12 <= exact <= c.auc_hi + 1e-12, (rows, scale, c.auc_lo, exact, c.auc_hi)   # (ties in p: at most the width)
            t_curve, t_sort = pair(curve, srt, args.warmup, args.repeats)
            emit(json.dumps({"case": "curve", "rows": rows, "logit_scale": scale, "repeats": args.repeats, "binary_curve": t_curve,
                             "torch_sort_cumsum": t_sort, "auc": c.auc, "auc_width": c.auc_hi - c.auc_lo}), args.out)
        ones = torch.ones(rows, device="cuda")
        y = (torch.arange(rows, device="cuda") % 2).to(torch.int32)
        t_ones, t_sort = pair(lambda: classification.binary_curve(ones, y, bins=10), lambda: sort_auc(ones, y), args.warmup, args.repeats)
        emit(json.dumps({"case": "curve_all_ones", "rows": rows, "repeats": args.repeats, "binary_curve": t_ones, "torch_sort_cumsum": t_sort}),
             args.out)


if __name__ == "__main__":
    main()
