#!/usr/bin/env python3
"""Times the model weights (d3p_stacking_weights, d3p_bb_pseudo_bma; d3p_amd.model_weights) with device events after a warm-up
(developer tool).

    python tools/time_model_weights.py [--reps 10] [--small]

At rows = 10^4 and 10^6 (--small: 10^4 only), M = 4 and 16, on a resident models x rows float32 matrix of the tests' form
(base_r + N(0, 0.5^2) + linspace(0, -0.3, M)):

  (a) stacking per evaluation: a run cut off at 256 updates (tol = 1e-300) over 257 evaluations, ALTERNATING with the torch float64
      composition of the same iteration over a float64 p computed once beforehand (den = w @ p, g = mean(p / den), w *= g; the
      composition neither forms f nor tests the gap, and is not synchronised with the host inside the 257 iterations);
  (b) stacking end to end at tol = 1e-7, max_iter = 20000, with the iteration count it took;
  (c) the bootstrap at B = 1000 against a chunked torch composition: per chunk of 65536 rows one (B, chunk) float64 Exponential(1)
      sample, its row sums and one matmul with the chunk of e; then z, the softmax and the mean.  (Another random stream: only the time
      is compared.)

Per line: microseconds (median, minimum and maximum over the repetitions) and the ratios of the medians.  Fails without a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random.debug as jax_random  # noqa: E402
from d3p_amd import model_weights as MW  # noqa: E402
from tools.time_waic import _line, _time_alternating  # noqa: E402

EVALS = 257
CHUNK = 65536


def _matrix(rows, M, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    base = -1.5 + torch.randn(rows, device="cuda", generator=g)
    e = base[None, :] + 0.5 * torch.randn((M, rows), device="cuda", generator=g) + torch.linspace(0.0, -0.3, M, device="cuda")[:, None]
    return e.contiguous()


def _torch_iterations(p, n):
    w = torch.full((p.shape[0],), 1.0 / p.shape[0], dtype=torch.float64, device=p.device)
    for _ in range(n):
        w = w * (p / (w @ p)).mean(dim=1)
    return w


def _torch_bootstrap(e64, B):
    M, rows = e64.shape
    T = torch.zeros((B, M), dtype=torch.float64, device=e64.device)
    S = torch.zeros((B,), dtype=torch.float64, device=e64.device)
    for lo in range(0, rows, CHUNK):
        part = e64[:, lo:lo + CHUNK]
        g = torch.empty((B, part.shape[1]), dtype=torch.float64, device=e64.device).exponential_(1.0)
        S += g.sum(dim=1)
        T += g @ part.T
    return torch.softmax(rows * T / S[:, None], dim=1).mean(dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    L.require_device()
    key = jax_random.PRNGKey(7)
    for rows in ((10_000,) if args.small else (10_000, 1_000_000)):
        for M in (4, 16):
            e = _matrix(rows, M)
            e64 = e.to(torch.float64)
            p = torch.exp(e64 - e64.max(dim=0).values)
            shape = f"rows={rows} M={M}"
            t_k, t_t = _time_alternating([lambda: MW.stacking_from_matrix(e, tol=1e-300, max_iter=EVALS - 1),
                                          lambda: _torch_iterations(p, EVALS)], args.reps)
            _line(f"stacking, {EVALS} evaluations {shape}", t_k, {"us_per_evaluation": round(t_k[0] / EVALS, 2),
                                                                  "torch_us_per_iteration": round(t_t[0] / EVALS, 2),
                                                                  "torch_over_this": round(t_t[0] / t_k[0], 2)})
            _line(f"torch float64 composition, {EVALS} iterations over a cached p {shape}", t_t)
            t_e = _time_alternating([lambda: MW.stacking_from_matrix(e)], max(3, args.reps // 3), warmup=1)[0]
            info = MW.stacking_from_matrix(e)[1].cpu().tolist()
            _line(f"stacking end to end, tol=1e-7 {shape}", t_e, {"n_iter": int(info[0]), "converged": bool(info[1]), "gap": info[2]})
            t_b, t_c = _time_alternating([lambda: MW.bootstrap_from_matrix(key, e, n_boot=1000), lambda: _torch_bootstrap(e64, 1000)],
                                         max(3, args.reps // 2), warmup=1)
            _line(f"bootstrap B=1000 {shape}", t_b, {"weights_per_s": round(1000 * rows / (t_b[0] * 1e-6)), "torch_over_this": round(t_c[0] / t_b[0], 2)})
            _line(f"torch chunked Exponential x matmul B=1000 {shape}", t_c)
            del e, e64, p


if __name__ == "__main__":
    main()
