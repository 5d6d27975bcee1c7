#!/usr/bin/env python3
"""Times d3p_vae_log_weights and held_out_density (d3p_amd.vae_density) with device events after a warm-up (developer tool).

    python tools/time_vae_density.py [--reps 20]

Shapes: 784 -> 400 -> 50 at B = 4096, n = 64 (the benchmark's batch) and the example's test split B = 512, n = 64.  Per shape, on
parameters and a batch prepared beforehand:

  (a) d3p_vae_log_weights (all draws in one slab, and in the slabs the 256 MiB default cap picks) and d3p_predict_vae at the same
      (B, n), ALTERNATING in one loop so that both see the same state of the machine: that call runs the same encoder, draws and
      decoder products and replaces the log-weight kernel by the Bernoulli draw;
  (b) k_vae_logw alone (d3p_vae_logw_rows) over all n B rows of logits composed beforehand -- its share of the whole call is the ratio
      of the medians -- and d3p_col_stats on the (n, B) matrix;
  (c) held_out_density end to end with and without the Pareto fit;
  (d) a torch composition of the same log weights from the same z: matmuls, softplus, the three sums in float32, then
      torch.logsumexp and the mean over the draws.

Per line: microseconds (median, minimum and maximum over the repetitions).  Fails without a GPU."""
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
from d3p_amd import modelling as M  # noqa: E402
from d3p_amd import vae_density as VD  # noqa: E402
from d3p_amd._lib import check, ptr, stream_ptr  # noqa: E402
from d3p_amd.models import VAEGuide, VAEModel  # noqa: E402


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


def _params(D, H, Z, g):
    shapes, n_dec = M._vae_leaf_shapes(L.VaeModel(D, H, Z, 1.0, 1.0, 0))
    leaves = [0.05 * torch.randn(s, device="cuda", generator=g) for s in shapes]
    return torch.cat([x.reshape(-1) for x in leaves]), leaves


def case(B, n, reps, D=784, H=400, Z=50):
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    flat, (V1, c1, V2, c2, W1, b1, Wl, bl, Ws, bs) = _params(D, H, Z, g)
    X = (torch.rand((B, D), device="cuda", generator=g) < 0.25).float()
    vm = L.VaeModel(D, H, Z, 1.0, 1.0, 0)
    model = VAEModel(Z, H)
    guide = VAEGuide(model)
    key = jr.PRNGKey(0)
    shape = f"784-400-50 B={B} n={n}"
    z = torch.empty((n, B, Z), device="cuda")
    logw = torch.empty((n, B), device="cuda")
    obs = torch.empty((n, B, D), dtype=torch.int32, device="cuda")
    dps_cap = VD._draws_per_slab(lib, vm, B, n, 256 << 20)
    ws = {k: torch.empty(int(lib.d3p_vae_log_weights_workspace(C.byref(vm), B, k)), dtype=torch.uint8, device="cuda") for k in {n, dps_cap}}
    pws = torch.empty(int(lib.d3p_predict_vae_workspace(C.byref(vm), B, n)), dtype=torch.uint8, device="cuda")

    def log_weights(dps):
        def run():
            check(lib.d3p_vae_log_weights(stream_ptr(), C.byref(vm), ptr(flat), ptr(X), B, ptr(key), n, 1, dps, ptr(z), ptr(logw), None, ptr(ws[dps]),
                                          ws[dps].numel()))
        return run

    def predict():
        check(lib.d3p_predict_vae(stream_ptr(), C.byref(vm), ptr(flat), ptr(X), B, ptr(key), n, 1, None, ptr(z), ptr(obs), ptr(pws), pws.numel()))

    t_one, t_cap, t_pred = _time_alternating([log_weights(n), log_weights(dps_cap), predict], reps)

    # the torch composition, from the same z and the same parameters
    def composition():
        sp = torch.nn.functional.softplus
        h = sp(X @ W1 + b1)
        zl, zs = h @ Wl + bl, h @ Ws + bs
        a = sp(z.reshape(n * B, Z) @ V1 + c1) @ V2 + c2
        px = (X.repeat(n, 1) * a - sp(a)).sum(1).reshape(n, B)
        pz = (-0.5 * z * z - 0.5 * math.log(2 * math.pi)).sum(2)
        u = (z - zl) * torch.exp(-zs)
        qz = (-0.5 * u * u - zs - 0.5 * math.log(2 * math.pi)).sum(2)
        lw = px + pz - qz
        return lw, torch.logsumexp(lw.double(), 0) - math.log(n), lw.double().mean(0)

    log_weights(n)()
    t_comp = _time_alternating([composition], max(3, reps // 4), warmup=1)[0]
    lw_t = composition()[0]
    diff = float((lw_t - logw).abs().max())

    # k_vae_logw alone (d3p_vae_logw_rows) over all n B rows, on logits and heads composed by torch from the same z
    sp = torch.nn.functional.softplus
    h = sp(X @ W1 + b1)
    zl, zs = (h @ Wl + bl).contiguous(), (h @ Ws + bs).contiguous()
    logits = (sp(z.reshape(n * B, Z) @ V1 + c1) @ V2 + c2).contiguous()
    lw_k = torch.empty(n * B, device="cuda")

    def kernel_alone():
        check(lib.d3p_vae_logw_rows(stream_ptr(), ptr(logits), ptr(X), ptr(z), ptr(zl), ptr(zs), n * B, B, D, Z, ptr(lw_k), None))

    t_kernel = _time_alternating([kernel_alone], reps)[0]
    del logits
    stats_out = torch.empty((4, B), dtype=torch.float64, device="cuda")

    def col_stats():
        check(lib.d3p_col_stats(stream_ptr(), ptr(logw), B, n, B, ptr(stats_out)))

    def density(k):
        return lambda: VD.held_out_density(key, n, model, guide, flat, X.reshape(B, D), z_dim=Z, hidden_dim=H, pareto_k=k)

    t_stats, t_full, t_nok = _time_alternating([col_stats, density(True), density(False)], reps)
    _line(f"d3p_vae_log_weights one slab {shape}", t_one, {"over_predict_vae": round(t_one[0] / t_pred[0], 3), "torch_over_this": round(t_comp[0] / t_one[0], 2),
                                                         "max_abs_diff_vs_torch": diff, "k_vae_logw_share_of_call": round(t_kernel[0] / t_one[0], 3)})
    _line(f"d3p_vae_log_weights slabs of {dps_cap} draws (256 MiB cap) {shape}", t_cap, {"workspace_MiB": round(ws[dps_cap].numel() / 2 ** 20, 1),
                                                                                       "one_slab_workspace_MiB": round(ws[n].numel() / 2 ** 20, 1)})
    _line(f"d3p_predict_vae {shape}", t_pred)
    _line(f"k_vae_logw alone, all n B rows (d3p_vae_logw_rows) {shape}", t_kernel, {"GB_per_s_of_logits": round(n * B * D * 4 / t_kernel[0] / 1e3, 1)})
    _line(f"torch composition (matmuls, softplus, logsumexp) {shape}", t_comp)
    _line(f"d3p_col_stats {shape}", t_stats)
    _line(f"held_out_density with pareto_k {shape}", t_full)
    _line(f"held_out_density without pareto_k {shape}", t_nok)


def slab_counts(B, n, reps, D=784, H=400, Z=50):
    """The whole call at draws_per_slab 1, 8 and n."""
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    flat, _ = _params(D, H, Z, g)
    X = (torch.rand((B, D), device="cuda", generator=g) < 0.25).float()
    vm = L.VaeModel(D, H, Z, 1.0, 1.0, 0)
    key = jr.PRNGKey(0)
    z = torch.empty((n, B, Z), device="cuda")
    logw = torch.empty((n, B), device="cuda")
    for dps in sorted({1, 8, n}):
        ws = torch.empty(int(lib.d3p_vae_log_weights_workspace(C.byref(vm), B, dps)), dtype=torch.uint8, device="cuda")

        def run():
            check(lib.d3p_vae_log_weights(stream_ptr(), C.byref(vm), ptr(flat), ptr(X), B, ptr(key), n, 1, dps, ptr(z), ptr(logw), None, ptr(ws), ws.numel()))

        _line(f"d3p_vae_log_weights draws_per_slab={dps} 784-400-50 B={B} n={n}", _time_alternating([run], reps)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slabs", action="store_true", help="also time the call at draws_per_slab 1, 8 and n")
    a = ap.parse_args()
    L.require_device()
    for B, n in ((4096, 64), (512, 64)):
        case(B, n, a.reps)
        if a.slabs:
            slab_counts(B, n, a.reps)


if __name__ == "__main__":
    main()
