"""Times DPSVI.run_steps of the logistic-regression path for a few model shapes (developer tool).
usage: python tools/time_logreg_shapes.py [--family {logreg,linreg,poisson}] [--shapes d:intercept:B,...] [--repeats R]
  ->  one line per shape: family, d, intercept, batch, median us per step over R timed runs (default 1)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import d3p_amd.random as rng
from d3p_amd.minibatch import subsample_batchify_data
from d3p_amd.models import Adam, AutoDiagonalNormal, LinearRegression, LogisticRegression, PoissonRegression, Trace_ELBO
from d3p_amd.svi import DPSVI, DPSVIState

def run(d, icpt, B, N=200000, steps=960, family="logreg", repeats=1):
    g = torch.Generator().manual_seed(0)
    X = torch.randn(N, d, generator=g).cuda()
    if family == "logreg":
        y = (torch.rand(N, generator=g) < 0.5).float().cuda()
        model = LogisticRegression(d, intercept=icpt)
    elif family == "linreg":
        y = torch.randn(N, generator=g).cuda()
        model = LinearRegression(d, intercept=icpt)
    else:
        y = torch.poisson(torch.ones(N), generator=g).cuda()
        model = PoissonRegression(d, intercept=icpt)
    svi = DPSVI(model, AutoDiagonalNormal(model), Adam(1e-3), Trace_ELBO(), 1.0, 1.0, num_obs_total=N)
    D = d + int(icpt)
    st = DPSVIState(svi.optim.init(torch.cat([torch.zeros(D), torch.full((D,), -2.0)]).cuda()), rng.PRNGKey(3), float(N))
    _, gb = subsample_batchify_data((X, y), B)
    st, _ = svi.run_steps(st, gb, rng.PRNGKey(4), 0, 96)
    st, _ = svi.run_steps(st, gb, rng.PRNGKey(4), 96, steps)  # (first call of a new shape / length pays one-off set-up)
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st1, losses = svi.run_steps(st, gb, rng.PRNGKey(4), 96, steps)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / steps * 1e6)
    times.sort()
    tag = "" if family == "logreg" and repeats == 1 else f"{family} "
    spread = "" if repeats == 1 else f" (min {times[0]:.2f} max {times[-1]:.2f}, {repeats} runs)"
    print(f"{tag}d={d} intercept={icpt} B={B}: {times[len(times) // 2]:.2f} us/step{spread}  loss {float(losses[-1]):.3f}", flush=True)

if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=["logreg", "linreg", "poisson"], default="logreg")
    ap.add_argument("--shapes", default=None, help="d:intercept:B,... (default: the built-in list)")
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    if a.shapes:
        for spec in a.shapes.split(","):
            d, icpt, B = spec.split(":")
            run(int(d), bool(int(icpt)), int(B), family=a.family, repeats=a.repeats)
        sys.exit(0)
    for d, icpt, B in ((4, True, 4096), (4, True, 256), (16, False, 4096), (512, False, 4096), (512, True, 4096), (256, False, 4096), (256, True, 4096), (64, True, 1024),
                       (1024, False, 4096), (1024, True, 4096), (100, False, 4096), (300, False, 4096), (2048, False, 4096)):
        run(d, icpt, B, family=a.family, repeats=a.repeats)
