"""Times DPSVI.update() with the logistic-regression example's OWN two-site guide (MeanFieldGuide; examples/logistic_regression.py:67-86)
against AutoDiagonalNormal over the same model (with intercept), on one resident batch, then DPSVI.run_steps() with that guide --
the native run loop against the stepwise route (get_batch + update per step) -- at (B, d) = (4096, 512) and (200, 4), the example's
default shape (developer tool).
    python tools/time_example_guide.py [B=4096] [d=512]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import d3p_amd.random as rng
from d3p_amd.models import Adam, AutoDiagonalNormal, LogisticRegression, MeanFieldGuide, Trace_ELBO
from d3p_amd.svi import DPSVI

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
d = int(sys.argv[2]) if len(sys.argv) > 2 else 512
N, steps = 200000, 300
g = torch.Generator().manual_seed(0)
X = torch.randn(B, d, generator=g).cuda(); y = (torch.rand(B, generator=g) < 0.5).float().cuda()
model = LogisticRegression(d, intercept=True)
for name, guide in (("AutoDiagonalNormal (fused step)", AutoDiagonalNormal(model)), ("MeanFieldGuide (the example's own guide)", MeanFieldGuide(model))):
    svi = DPSVI(model, guide, Adam(1e-3), Trace_ELBO(), 1.0, 1.0, num_obs_total=N)
    st = svi.init(rng.PRNGKey(3), X, y)
    for phase in range(2):
        s = st
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for t in range(steps):
            s, loss = svi.update(s, X, y)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print(f"{name}: {dt / steps * 1e6:.1f} us per update (B = {B}, d = {d} + intercept), loss {float(loss):.4g}", flush=True)
svi_staged = svi        # (the last one: MeanFieldGuide) -- the reference's five-stage composition on the same guide
for phase in range(2):
    s = st
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for t in range(steps):
        s, loss = svi_staged._update_staged(s, X, y)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
print(f"MeanFieldGuide through the five-stage composition: {dt / steps * 1e6:.1f} us per update, loss {float(loss):.4g}", flush=True)


# run_steps: the native loop (D3P_GUIDE_EXP_SITES) against get_batch + update per step, Feistel batches from a resident table
from d3p_amd.minibatch import subsample_batchify_data
for (Bs, ds, Ns, run) in ((4096, 512, 100000, 1024), (200, 4, 10000, 1024)):
    Xt = torch.randn(Ns, ds, generator=g).cuda(); yt = (torch.rand(Ns, generator=g) < 0.5).float().cuda()
    m2 = LogisticRegression(ds, intercept=True)
    _, gb = subsample_batchify_data((Xt, yt), Bs)
    for name, guide in (("AutoDiagonalNormal", AutoDiagonalNormal(m2)), ("MeanFieldGuide", MeanFieldGuide(m2))):
        svi = DPSVI(m2, guide, Adam(1e-3), Trace_ELBO(), 1.0, 1.0, num_obs_total=Ns)
        st = svi.init(rng.PRNGKey(5), Xt[:Bs], yt[:Bs])
        forms = [("native", svi.run_steps)]
        if name == "MeanFieldGuide":
            forms.append(("stepwise", svi._run_steps_stepwise))
        for form, fn in forms:
            n = run if form == "native" else 200
            for phase in range(2):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                s, losses = fn(st, gb, rng.PRNGKey(6), 0, n)
                torch.cuda.synchronize(); dt = time.perf_counter() - t0
            print(f"run_steps {name} ({form}, {n} steps): {dt / n * 1e6:.2f} us per step (B = {Bs}, d = {ds} + intercept), "
                  f"last loss {float(losses[-1]):.4g}", flush=True)
