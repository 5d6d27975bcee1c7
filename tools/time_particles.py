"""Device-event timing of DPSVI.run_steps with Trace_ELBO(num_particles=K): Feistel batches, B = 4096, 200 steps after a warm-up
run, K in {1, 2, 4, 8} x d in {4, 64, 512, 513, 1024}; then DPSVI.update calls at d = 512 + intercept under the example's own
MeanFieldGuide.  K = 1 is the single-particle default (chained launches); K > 1 runs k_logreg_particles + k_finalize per step.
Prints one line per configuration (us per step)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import d3p_amd._lib as L
import d3p_amd.random as rng
from d3p_amd.minibatch import subsample_batchify_data
from d3p_amd.models import Adam, AutoDiagonalNormal, LogisticRegression, MeanFieldGuide, Trace_ELBO
from d3p_amd.svi import DPSVI, DPSVIState


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1), out


def main():
    lib = L.load()
    L.require_device()
    dev = torch.device("cuda:0")
    N, B, steps = 100_000, 4096, 200
    Ks = [int(k) for k in os.environ.get("D3P_TP_K", "1,2,4,8").split(",")]
    ds = [int(d) for d in os.environ.get("D3P_TP_D", "4,64,512,513,1024").split(",")]
    for d in ds:
        X = torch.empty((N, d), device=dev)
        y = torch.empty(N, device=dev)
        L.check(lib.d3p_synth_logreg(L.stream_ptr(), 123, 0, N, d, L.ptr(X), L.ptr(y)))
        _, gb = subsample_batchify_data((X, y), B)
        for K in Ks:
            model = LogisticRegression(d)
            svi = DPSVI(model, AutoDiagonalNormal(model), Adam(1e-3), Trace_ELBO(num_particles=K), 1.0, 1.0, N=N)
            st = DPSVIState(svi.optim.init(torch.cat([torch.zeros(d, device=dev), torch.full((d,), -2.25, device=dev)])),
                            rng.PRNGKey(0), float(N))
            st, _ = svi.run_steps(st, gb, rng.PRNGKey(1), 0, 20)
            us, (st2, losses) = timed(lambda: svi.run_steps(st, gb, rng.PRNGKey(1), 20, steps, check_status=False))
            assert svi.last_run_status() == (False, False) and bool(torch.isfinite(losses).all())
            print(f"run_steps d={d} K={K}: {us / steps:.2f} us/step", flush=True)
        del X, y
    d = 512
    X = torch.empty((B, d), device=dev)
    y = torch.empty(B, device=dev)
    L.check(lib.d3p_synth_logreg(L.stream_ptr(), 7, 0, B, d, L.ptr(X), L.ptr(y)))
    for K in Ks:
        model = LogisticRegression(d, intercept=True)
        svi = DPSVI(model, MeanFieldGuide(model), Adam(1e-3), Trace_ELBO(num_particles=K), 1.0, 1.0, N=N)
        st = DPSVIState(svi.optim.init(torch.zeros(2 * d + 2, device=dev)), rng.PRNGKey(0), float(N))
        st, _ = svi.update(st, X, y)
        holder = [st]

        def step():
            holder[0], loss = svi.update(holder[0], X, y)
            return loss
        us, _ = timed(step, reps=50)
        print(f"update MeanFieldGuide d=512+intercept B={B} K={K}: {us / 50:.2f} us/call", flush=True)


if __name__ == "__main__":
    main()
