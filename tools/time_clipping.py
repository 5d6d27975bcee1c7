#!/usr/bin/env python3
"""Times the clipping diagnostics (d3p_amd.clipping, d3p_logreg_grad_norms, d3p_norm_profile) with device events after a warm-up
(developer tool).

    python tools/time_clipping.py [--reps 20] [--small]

  (a) per family at d = 512 + intercept, 10^6 rows and at the examples' d = 4, 10^4 rows (--small: the latter only), alternating:
      clipping.gradient_norms; d3p_logreg_grad_norms alone with the noise from the key and with the noise read from memory (the
      difference is the cost of generating rows x D normals); d3p_logreg_px_grads + torch.linalg.vector_norm at the largest power of
      two of rows whose rows x 2 D tensor stays within 1 GiB, scaled per row; and a device copy of X, whose half is the time to read
      X once at the box's copy rate;
  (b) at n = 10^6 and 10^7 |normal| values, 1 threshold, 4 probabilities, alternating: clipping.norm_profile (two calls of the entry
      and two host reads), d3p_norm_profile alone (one call with the positions given), and torch.sort + two gathers and a lerp per
      probability.

Per line: microseconds (median, minimum and maximum over the repetitions) and the ratios of the medians.  Fails without a GPU."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random as rng_suite  # noqa: E402
from d3p_amd import clipping as CL  # noqa: E402
from d3p_amd._lib import check, ptr, stream_ptr  # noqa: E402
from d3p_amd.intervals import positions  # noqa: E402
from d3p_amd.models import Adam, AutoDiagonalNormal, Trace_ELBO  # noqa: E402
from d3p_amd.svi import DPSVI, DPSVIState  # noqa: E402
from tools.time_loglik import _problem  # noqa: E402
from tools.time_waic import _line, _time_alternating  # noqa: E402

PROBS = (0.5, 0.9, 0.95, 0.99)
ROWS_TENSOR_BYTES = 1 << 30


def gradient_norm_cases(reps, shapes):
    lib = L.load()
    for d, rows in shapes:
        D = d + 1
        for family in ("logistic", "linear", "poisson"):
            model, _, X, y, lat = _problem(family, d, rows, 1)
            svi = DPSVI(model, AutoDiagonalNormal(model), Adam(1e-3), Trace_ELBO(), 1.0, 1.0, num_obs_total=rows, rng_suite=rng_suite)
            params = torch.cat([lat[0], torch.full((D,), -1.5, device="cuda")]).contiguous()
            st = DPSVIState(svi.optim.init(params), rng_suite.PRNGKey(0), float(rows))
            ms = svi._model_struct(d, {}, st.observation_scale)
            jk = rng_suite.convert_to_jax_rng_key(rng_suite.split(st.rng_key, 3)[1]).contiguous()
            norms = torch.empty(rows, device="cuda")
            ws = torch.empty(int(lib.d3p_logreg_grad_norms_workspace(C.byref(ms), rows)), dtype=torch.uint8, device="cuda")
            eps = torch.randn((rows, D), device="cuda")
            B = 1
            while 2 * B <= rows and 2 * B * 2 * D * 4 <= ROWS_TENSOR_BYTES:
                B *= 2
            px = torch.empty((B, 2 * D), device="cuda")
            px_loss, meta = torch.empty(B, device="cuda"), torch.empty(2, device="cuda")
            pws = torch.empty(int(lib.d3p_logreg_px_grads_workspace(C.byref(ms), B)), dtype=torch.uint8, device="cuda")
            Xcopy = torch.empty_like(X)

            def entry(e, k):
                check(lib.d3p_logreg_grad_norms(stream_ptr(), C.byref(ms), ptr(params), ptr(X), ptr(y), rows, 0, rows, ptr(e), ptr(k), ptr(norms),
                                                None, ptr(ws), ws.numel()))

            def rows_then_norm():
                check(lib.d3p_logreg_px_grads(stream_ptr(), C.byref(ms), ptr(params), ptr(X), ptr(y), None, B, None, ptr(jk), ptr(px_loss),
                                              ptr(px), ptr(meta), ptr(pws), pws.numel()))
                return torch.linalg.vector_norm(px, dim=1)

            t_py, t_key, t_mem, t_rows, t_copy = _time_alternating(
                [lambda: CL.gradient_norms(svi, st, X, y), lambda: entry(None, jk), lambda: entry(eps, None), rows_then_norm,
                 lambda: Xcopy.copy_(X)], reps)
            shape = f"{family} d={d} rows={rows}"
            per_row = t_rows[0] * rows / B
            x_bytes = rows * d * 4
            _line(f"clipping.gradient_norms {shape}", t_py)
            _line(f"d3p_logreg_grad_norms alone, noise from the key {shape}", t_key,
                  {"rows_path_over_this": round(per_row / t_key[0], 2), "over_reading_X_once": round(t_key[0] / (t_copy[0] / 2), 2),
                   "normals_per_s": round(rows * D / (t_key[0] * 1e-6))})
            _line(f"d3p_logreg_grad_norms alone, noise from memory {shape}", t_mem, {"key_over_memory": round(t_key[0] / t_mem[0], 2)})
            _line(f"d3p_logreg_px_grads + vector_norm at {B} rows {shape}", t_rows, {"us_scaled_to_all_rows": round(per_row, 1),
                                                                                    "rows_tensor_bytes": B * 2 * D * 4})
            _line(f"device copy of X {shape}", t_copy, {"copy_bytes_per_s": round(2 * x_bytes / (t_copy[0] * 1e-6)),
                                                        "us_to_read_X_once": round(t_copy[0] / 2, 1)})
            del X, y, eps, px, Xcopy, norms
            torch.cuda.empty_cache()


def _torch_profile(v, pos):
    s = torch.sort(v).values
    out = []
    for lo, g in pos:
        a, b = s[lo], s[min(lo + 1, v.numel() - 1)]
        dd = b - a
        out.append(a + dd * g if g < 0.5 else b - dd * (1.0 - g))
    return torch.stack(out)


def profile_cases(reps, sizes):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    for n in sizes:
        v = torch.randn(n, device="cuda", generator=g).abs()
        pos = positions(PROBS, n)
        out = torch.empty(29, dtype=torch.int64, device="cuda")
        ws = torch.empty(int(lib.d3p_norm_profile_workspace(n)), dtype=torch.uint8, device="cuda")
        thr = (C.c_float * 1)(1.0)
        lo = (C.c_uint64 * len(pos))(*[p[0] for p in pos])
        gg = (C.c_double * len(pos))(*[p[1] for p in pos])

        def entry():
            check(lib.d3p_norm_profile(stream_ptr(), ptr(v), n, 1, thr, len(pos), lo, gg, ptr(out), ptr(ws), ws.numel()))

        t_py, t_entry, t_sort = _time_alternating([lambda: CL.norm_profile(v, (1.0,), PROBS), entry, lambda: _torch_profile(v, pos)], reps)
        entry()
        same = bool(torch.equal(out[21:25].view(torch.float64).float(), _torch_profile(v.double(), pos).float()))
        _line(f"clipping.norm_profile n={n}", t_py)
        _line(f"d3p_norm_profile alone n={n} m=1 Q=4", t_entry, {"torch_sort_over_this": round(t_sort[0] / t_entry[0], 2),
                                                                "values_per_s": round(n / (t_entry[0] * 1e-6)), "equals_float64_torch": same})
        _line(f"torch.sort + gathers + lerp n={n}", t_sort)
        del v
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="the examples' shape and n = 10^6 only")
    a = ap.parse_args()
    L.require_device()
    gradient_norm_cases(a.reps, ((4, 10_000),) if a.small else ((512, 1_000_000), (4, 10_000)))
    profile_cases(a.reps, (1_000_000,) if a.small else (1_000_000, 10_000_000))


if __name__ == "__main__":
    main()
