"""No entry reads stale workspace bytes or writes past its workspace (include/d3p_hip.h, "Workspaces"; DESIGN.md, "Workspace contract").

Every training and sampling entry takes a caller-supplied workspace; Python hands it ``torch.empty`` memory, which inside one pytest
process usually holds the correct intermediates of the previous, similar test.  Here every scenario runs on workspaces that
tests/workspace_harness.py pre-fills -- zeros, 0xFF bytes (NaN floats, -1 integers, maximal counters and tags), the largest finite
float, random bytes, the image a DONOR run left (the same entry and shapes, another key, other parameters, other data, another step
count: every tag and counter in it looks valid) and that image rolled by 256 bytes -- between two guard bands, at exactly the size the
``d3p_*_workspace()`` function declares.  Per scenario, on RAW BYTES (NaN equals NaN) of every output -- losses, the new state's
parameters, moments, step counter and key, any other returned tensor:

  (a) the run under ``zero`` equals the unpatched public call (which the oracle-pinned tests check) bit for bit; the wrappers that
      allocate with ``torch.empty`` themselves are the same public calls in both runs (their module allocates from the harness in the
      guarded one); only ``d3p_poisson_select_batch``, which has no wrapper of its own, is called directly;
  (b) the run under every other fill equals the ``zero`` run bit for bit;
  (c) every guard is intact after every run;
  (d) runs: ``last_run_status()`` reports no abort and no non-finite flag, and no fallback warning is raised;
  (e) for every public call of every scenario: a workspace one byte short is refused with a ``D3PError`` that names the workspace,
      and state, outputs, interior and guards are byte-identical to before the call: nothing was launched.

The entries promise fixed summation orders and integer atomics only, so equality is the assertion: no tolerance anywhere.  Shapes are
the smallest that reach each kernel form, taken from the tests that name the form they reach (test_gpu_production_kernels.py,
test_gpu_dpsvi.py, test_gpu_particles_edges.py, test_gpu_example_guide_run.py, test_gpu_gmm_update_edges.py, test_gpu_vae.py)."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import workspace_harness as H

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------- inputs
class V:
    """The two variants of a scenario: the run under test and its donor (another key, other parameters, other data, another step
    count -- the same entry and the same shapes, so the same workspace layout)."""

    def __init__(self, donor):
        self.donor = bool(donor)
        self.seed = 1000 if donor else 0          # added to every data / parameter seed
        self.key = 77 if donor else 0             # added to every PRNG key seed

    def steps(self, n):
        return n + 3 if self.donor else n


MAIN, DONOR = V(False), V(True)


@functools.lru_cache(maxsize=8)
def _table(N, d, seed, labels="bernoulli"):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g) / max(1.0, d ** 0.5) * 2.0
    if labels == "bernoulli":
        y = (torch.rand(N, generator=g) < 0.5).float()
    elif labels == "linear":
        y = torch.randn(N, generator=g)
    else:
        y = torch.poisson(torch.full((N,), 1.5), generator=g)
    return X.cuda().contiguous(), y.cuda().contiguous()


def _mask(B, seed):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) < 0.7


def _logreg_svi(d, icpt, N, family="logistic", K=1, guide="auto"):
    from d3p_amd.models import (Adam, AutoDiagonalNormal, LinearRegression, LogisticRegression, MeanFieldGuide, PoissonRegression,
                                Trace_ELBO)
    from d3p_amd.svi import DPSVI
    if family == "logistic":
        model = LogisticRegression(d, prior_scale=1.0, intercept=icpt, intercept_prior_scale=2.0)
    elif family == "linear":
        model = LinearRegression(d, prior_scale=1.5, intercept=icpt, intercept_prior_scale=2.5, obs_scale=0.8)
    else:
        model = PoissonRegression(d, prior_scale=1.5, intercept=icpt, intercept_prior_scale=2.5)
    g = MeanFieldGuide(model) if guide == "sites" else AutoDiagonalNormal(model)
    return DPSVI(model, g, Adam(1e-2), Trace_ELBO(num_particles=K), 1.0, 0.7, num_obs_total=N)


def _logreg_state(svi, D, N, v, seed, sites=False):
    import d3p_amd.random as rng
    from d3p_amd.svi import DPSVIState
    r = np.random.default_rng(seed + v.seed)
    if sites:   # tree order [intercept_loc, intercept_std_log, w_loc, w_std_log] (D = d + 1)
        p = np.concatenate([[0.3], [-1.2], 0.2 * r.normal(size=D - 1), -1.0 + 0.3 * r.normal(size=D - 1)])
    else:
        p = np.concatenate([0.1 * r.normal(size=D), -2.0 + 0.2 * r.normal(size=D)])
    return _watch(DPSVIState(svi.optim.init(torch.tensor(p.astype(np.float32)).cuda()), rng.PRNGKey(seed + v.key), float(N)))


_WATCHED = []   # (tensor, clone at creation) of every state a scenario built: the refusal test compares them afterwards


def _watch(st):
    for t in tuple(st.optim_state) + (st.rng_key,):
        if isinstance(t, torch.Tensor):
            _WATCHED.append((t, t.clone()))
    return st


def _state_out(out, name, st):
    step, params, m, v = st.optim_state
    out[name + ".step"], out[name + ".params"], out[name + ".m"], out[name + ".v"] = step, params, m, v
    out[name + ".key"] = st.rng_key


def _tree_out(out, name, tree):
    for k in sorted(tree):
        out[f"{name}.{k}"] = tree[k]


# ---------------------------------------------------------------------------------------------------------------- scenarios
# A scenario is fn(v, rec) -> {name: tensor}: every public call on a FRESH DPSVI object (its workspaces are handed out, and filled,
# anew); `rec` is the harness's recorder (None in the unpatched run), used by the scenarios that pass a workspace themselves.
def logreg_step(B, d, icpt, masked, family="logistic", K=1):
    """DPSVI.update (d3p_dpvi_logreg_run_from, one step, on-chip noise) and _compute_per_example_gradients (d3p_logreg_px_grads*)."""
    def fn(v, rec):
        import d3p_amd.random as rng
        N, D = 5000, d + int(icpt)
        X, y = _table(B, d, 11 + B + d + v.seed, {"logistic": "bernoulli", "linear": "linear", "poisson": "counts"}[family])
        mask = _mask(B, 5 + B + v.seed).cuda() if masked else True
        out = {}
        svi = _logreg_svi(d, icpt, N, family, K)
        st = _logreg_state(svi, D, N, v, 21)
        new_st, loss = svi.update(st, X, y, mask=mask)
        out["update.loss"] = loss
        _state_out(out, "update", new_st)
        svi = _logreg_svi(d, icpt, N, family, K)
        _, px_loss, grads, n, f = svi._compute_per_example_gradients(st, rng.PRNGKey(31 + v.key), X, y, mask=mask)
        out["px.loss"], out["px.n"], out["px.factor"] = px_loss, n, f
        _tree_out(out, "px.grads", grads)
        return out
    return fn


def logreg_run(B, d, icpt, steps, sampler="feistel", family="logistic", K=1, guide="auto", N=5000):
    """DPSVI.run_steps (k_run_init -> sampler -> step launches -> k_flush) through the form the shape selects."""
    def fn(v, rec):
        import d3p_amd.random as rng
        from d3p_amd.minibatch import poisson_batchify_data, subsample_batchify_data
        D = d + int(icpt)
        X, y = _table(N, d, 13 + B + d + v.seed, {"logistic": "bernoulli", "linear": "linear", "poisson": "counts"}[family])
        svi = _logreg_svi(d, icpt, N, family, K, guide)
        st = _logreg_state(svi, D, N, v, 23, sites=guide == "sites")
        gb = (subsample_batchify_data((X, y), B) if sampler == "feistel" else poisson_batchify_data((X, y), B / N, 0.99))[1]
        new_st, losses = svi.run_steps(st, gb, rng.PRNGKey(41 + v.key), 2, v.steps(steps))
        assert svi.last_run_status() == (False, False), svi.last_abort_code()     # (d)
        out = {"run.losses": losses}
        _state_out(out, "run", new_st)
        return out
    return fn


def logreg_exchange(B, icpt, steps):
    """The data-parallel UPDATER form (tagged state words) on a world of one rank, as
    test_chain_kernel_exchange_on_one_rank_vs_oracle_across_a_launch_boundary sets it up; the engine keeps a workspace it is given."""
    def fn(v, rec):
        import d3p_amd._lib as L
        import d3p_amd.random as rng
        from d3p_amd import dist as ddist
        N, d = 5000, 512
        D = d + int(icpt)
        X, y = _table(N, d, 14 + B + v.seed)
        svi = _logreg_svi(d, icpt, N)
        st = _logreg_state(svi, D, N, v, 25)
        eng = ddist.FusedHipEngine(svi, X, y, N, 0, N, L.D3P_BATCH_FEISTEL, B)
        if rec is not None:
            model = svi._model_struct(d, {}, float(N))
            src = L.BatchSource(L.D3P_BATCH_FEISTEL, B, 0.0, 0, None, None, None, N, 0, N)
            mine = rec.take(L.load().d3p_dpvi_logreg_workspace(C.byref(model), C.byref(src)), DEV, "ws").interior
            given, setup = mine.data_ptr(), eng._setup_lean

            def setup_then_my_workspace(*a, **k):     # (the engine replaces a buffer it finds too small: the refusal is the library's to make)
                ok = setup(*a, **k)
                eng.ws = mine
                return ok
            eng._setup_lean = setup_then_my_workspace
        comm = ddist.XchgComm(2 * D + 4)
        try:
            new_st, losses = ddist.run_steps_native(eng, st, rng.PRNGKey(43 + v.key), 2, v.steps(steps), comm=comm)
            torch.cuda.synchronize()
            code, nonfinite = ddist.native_run_status(eng)
        finally:
            comm.close()
        assert rec is None or eng.ws.data_ptr() == given, "the engine did not run on the workspace it was given"
        assert (code, bool(nonfinite)) == (0, False), L.describe_abort(code)          # (d)
        out = {"run.losses": losses}
        _state_out(out, "run", new_st)
        return out
    return fn


def logreg_evaluate(B, d, icpt, K=1, guide="auto"):
    def fn(v, rec):
        N, D = 5000, d + int(icpt)
        X, y = _table(B, d, 15 + B + d + v.seed)
        svi = _logreg_svi(d, icpt, N, K=K, guide=guide)
        st = _logreg_state(svi, D, N, v, 27, sites=guide == "sites")
        return {"evaluate.loss": svi.evaluate(st, X, y)}
    return fn


def _gmm_svi(K, d, N):
    from d3p_amd.models import Adam, GaussianMixtureGuide, GaussianMixtureModel, Trace_ELBO
    from d3p_amd.svi import DPSVI
    model = GaussianMixtureModel()
    return DPSVI(model, GaussianMixtureGuide(model), Adam(1e-2), Trace_ELBO(), 20.0, 0.7, k=K, d=d, num_obs_total=N)


def _gmm_state(svi, K, d, N, v, seed):
    import d3p_amd.random as rng
    from d3p_amd.svi import DPSVIState
    r = np.random.default_rng(seed + v.seed)
    p = np.concatenate([r.normal(size=K) * 0.4, r.normal(size=K * d) * 2]).astype(np.float32)
    return _watch(DPSVIState(svi.optim.init(torch.tensor(p).cuda()), rng.PRNGKey(seed + v.key), float(N)))


def gmm_all(K, d, B):
    """The mixture model: update (masked and not), run_steps over 7 steps, the per-example gradients, evaluate."""
    def fn(v, rec):
        import d3p_amd.random as rng
        from d3p_amd.minibatch import subsample_batchify_data
        N = 2000
        X = (_table(N, d, 17 + K + d + v.seed)[0] * 3).contiguous()
        Xb = X[:B].contiguous()
        out = {}
        for name, mask in (("update", True), ("update_masked", _mask(B, 7 + v.seed).cuda())):
            svi = _gmm_svi(K, d, N)
            new_st, loss = svi.update(_gmm_state(svi, K, d, N, v, 51), Xb, mask=mask)
            out[name + ".loss"] = loss
            _state_out(out, name, new_st)
        svi = _gmm_svi(K, d, N)
        gb = subsample_batchify_data((X,), B)[1]
        new_st, losses = svi.run_steps(_gmm_state(svi, K, d, N, v, 52), gb, rng.PRNGKey(53 + v.key), 1, v.steps(7))
        out["run.losses"] = losses
        _state_out(out, "run", new_st)
        svi = _gmm_svi(K, d, N)
        st = _gmm_state(svi, K, d, N, v, 54)
        _, px_loss, grads, n, f = svi._compute_per_example_gradients(st, rng.PRNGKey(55 + v.key), Xb, mask=_mask(B, 9 + v.seed).cuda())
        out["px.loss"], out["px.n"], out["px.factor"] = px_loss, n, f
        _tree_out(out, "px.grads", grads)
        svi = _gmm_svi(K, d, N)
        out["evaluate.loss"] = svi.evaluate(st, Xb)
        return out
    return fn


def gmm_run(K, d, B, steps):
    """A mixture-model run longer than one prepared batch of 64 steps: the second slot / noise set and the key chain between batches."""
    def fn(v, rec):
        import d3p_amd.random as rng
        from d3p_amd.minibatch import subsample_batchify_data
        N = 2000
        X = (_table(N, d, 17 + K + d + v.seed)[0] * 3).contiguous()
        svi = _gmm_svi(K, d, N)
        gb = subsample_batchify_data((X,), B)[1]
        new_st, losses = svi.run_steps(_gmm_state(svi, K, d, N, v, 56), gb, rng.PRNGKey(57 + v.key), 1, v.steps(steps))
        out = {"run.losses": losses}
        _state_out(out, "run", new_st)
        return out
    return fn


def _vae_svi(Z, H, H2, N):
    from d3p_amd.models import Adam, Trace_ELBO, VAEGuide, VAEModel
    from d3p_amd.svi import DPSVI
    model = VAEModel(scale=1.0 / N)
    return DPSVI(model, VAEGuide(model), Adam(1e-3), Trace_ELBO(), 10.0, 0.8, num_obs_total=N, z_dim=Z, hidden_dim=(H, H2) if H2 else H)


@functools.lru_cache(maxsize=4)
def _images(N, D, seed, grey):
    u = torch.rand(N, D, generator=torch.Generator().manual_seed(seed))
    return (u if grey else (u < 0.3).float()).cuda().contiguous()    # grey: not exactly bf16; binarised: exactly bf16


def vae_all(B, D, H, Z, H2, grey=False):
    """The VAE: update, run_steps over 4 steps, evaluate.  ``grey``: a batch that is not exactly bf16 (the other value of the
    exactness word of the bf16 pipe's first product)."""
    def fn(v, rec):
        import d3p_amd.random as rng
        from d3p_amd.minibatch import subsample_batchify_data
        N = 300
        X = _images(N, D, 61 + D + v.seed, grey)
        Xb = X[:B].contiguous()
        out = {}
        svi = _vae_svi(Z, H, H2, N)
        st = _watch(svi.init(rng.PRNGKey(62 + v.key), Xb))
        new_st, loss = svi.update(st, Xb)
        out["update.loss"] = loss
        _state_out(out, "update", new_st)
        svi = _vae_svi(Z, H, H2, N)
        gb = subsample_batchify_data((X,), B)[1]
        new_st, losses = svi.run_steps(st, gb, rng.PRNGKey(63 + v.key), 1, v.steps(4))
        out["run.losses"] = losses
        _state_out(out, "run", new_st)
        svi = _vae_svi(Z, H, H2, N)
        out["evaluate.loss"] = svi.evaluate(st, Xb)
        return out
    return fn


# ---- entries whose Python wrappers allocate workspace and outputs with torch.empty themselves: the PUBLIC wrapper is called in the
# unpatched run and in the guarded runs alike; in the guarded runs the wrapper's module allocates from the recorder
# (H.guarded_empty), so the entry runs on a guarded, pre-filled workspace and writes into guarded outputs
class _guarded_module:
    """with _guarded_module(rec, module, tag): ... -- nothing in the unpatched run (rec is None)."""

    def __init__(self, rec, module, tag):
        self.rec, self.module, self.tag, self.mp = rec, module, tag, None

    def __enter__(self):
        if self.rec is not None:
            self.mp = pytest.MonkeyPatch()
            H.guarded_empty(self.mp, self.module, self.rec, self.tag)

    def __exit__(self, *exc):
        if self.mp is not None:
            self.mp.undo()


def _buf(rec, nbytes, tag, dtype, output=False):
    """nbytes of guarded memory from the recorder as a `dtype` tensor -- or plain zeroed memory in the unpatched run."""
    if rec is None:
        return torch.zeros(int(nbytes), dtype=torch.uint8, device=DEV).view(dtype)
    return rec.take(nbytes, DEV, tag, output=output).interior.view(dtype)


def poisson_select(N):
    """d3p_poisson_select_rng through poisson_batchify_data's get_batch: the rows of a table that holds its own row numbers, i.e. the
    selected indices (descending, zero beyond the valid count), and the mask."""
    def fn(v, rec):
        import d3p_amd.random as rng
        from d3p_amd import minibatch
        table = torch.arange(N, dtype=torch.float32, device=DEV).reshape(N, 1)
        get_batch = minibatch.poisson_batchify_data((table,), 0.3, max(N // 2, 1))[1]
        with _guarded_module(rec, minibatch, "poisson"):
            (rows,), mask = get_batch(3, rng.PRNGKey(71 + v.key))
        return {"rows": rows, "mask": mask}
    return fn


def poisson_select_batch(N, steps):
    """d3p_poisson_select_batch over `steps` draws (no Python wrapper of its own: the run loops call it inside their carve), called
    directly with the outputs inside guards; the unpatched run is the same call on plain memory."""
    def fn(v, rec):
        import d3p_amd._lib as L
        import d3p_amd.random as rng
        lib = L.load()
        q, cutoff = np.float32(0.3), max(N // 2, 1)
        per = lib.d3p_poisson_select_workspace(N)
        keys = torch.stack([rng.fold_in(rng.PRNGKey(71 + v.key), t).reshape(16) for t in range(steps)]).contiguous()
        ws = _buf(rec, per * steps, "poisson", torch.uint8)
        idx = _buf(rec, 4 * cutoff * steps, "out.idx", torch.uint32, output=True)
        counts = _buf(rec, 8 * steps, "out.counts", torch.uint32, output=True)
        L.check(lib.d3p_poisson_select_batch(L.stream_ptr(), 0, L.ptr(keys), 16, float(q), N, cutoff, 0, L.ptr(idx), cutoff,
                                             L.ptr(counts), 2, steps, L.ptr(ws), ws.numel()))
        return {"idx": idx, "counts": counts}
    return fn


def adadp(P):
    """d3p_adadp_step through ADADP.update: an even step (stores x_prev / x_stepped, writes no partials), then an odd one (reads them),
    each call with a workspace of its own."""
    def fn(v, rec):
        from d3p_amd import optimizers
        g = torch.Generator().manual_seed(81 + P + v.seed)
        x, grads = torch.randn(P, generator=g).cuda(), [torch.randn(P, generator=g).cuda() for _ in range(2)]
        _WATCHED.extend((a, a.clone()) for a in [x] + grads)
        opt = optimizers.ADADP(step_size=0.05, tol=1.0, stability_check=True)
        state = (4 if v.donor else 0, (x, 0.05, torch.zeros_like(x), x))
        out = {}
        for t in range(2):
            with _guarded_module(rec, optimizers, "adadp"):
                state = opt.update(grads[t], state)
            i, (x_t, lr_t, xs_t, xp_t) = state
            _WATCHED.extend((a, a.clone()) for a in (x_t, lr_t, xs_t, xp_t))     # (the state the next call starts from)
            out.update({f"x{t}": x_t, f"lr{t}": lr_t, f"xs{t}": xs_t, f"xp{t}": xp_t, f"step{t}": torch.tensor([int(i)], dtype=torch.int32)})
        return out
    return fn


def _vae_inputs(v, B, D, H, Z):
    import d3p_amd._lib as L
    from d3p_amd.models import VAEGuide, VAEModel
    vm = L.VaeModel(D, H, Z, 1.0, 1.0, 0)
    g = torch.Generator().manual_seed(97 + v.seed)
    flat = (0.3 * torch.randn(int(L.load().d3p_vae_num_params(C.byref(vm))), generator=g)).cuda()
    X = (torch.rand(B, D, generator=g) < 0.4).float().cuda()
    key = torch.tensor([1234 + v.key, 5678], dtype=torch.uint32, device=DEV)
    model = VAEModel(Z, H)
    return model, VAEGuide(model), flat, X, key


def predict_vae(B, n):
    """d3p_predict_vae, posterior form (encoder -> z -> decoder -> Bernoulli draws), through sample_multi_posterior_predictive."""
    def fn(v, rec):
        from d3p_amd import modelling
        D, H, Z = 12, 7, 3
        model, guide, flat, X, key = _vae_inputs(v, B, D, H, Z)
        with _guarded_module(rec, modelling, "predict_vae"):
            res = modelling.sample_multi_posterior_predictive(key, n, model, (B, Z, H, D), guide, (X, Z, H), flat)
        return {"z": res["z"], "obs": res["obs"]}
    return fn


def vae_log_weights(B, n, dps):
    """d3p_vae_log_weights over more than one slab, through log_importance_weights (with the per-site parts)."""
    def fn(v, rec):
        from d3p_amd import vae_density
        D, H, Z = 12, 7, 3
        model, guide, flat, X, key = _vae_inputs(v, B, D, H, Z)
        assert n * B > 96 and n // max(dps, -(-97 // B)) >= 2, "the case must run as at least two slabs"
        with _guarded_module(rec, vae_density, "vae_log_weights"):
            logw, sites = vae_density.log_importance_weights(key, n, model, guide, flat, X, z_dim=Z, hidden_dim=H, return_sites=True,
                                                             draws_per_slab=dps)
        return {"z": sites["z"], "logw": logw, "log_px": sites["log_px"], "log_pz": sites["log_pz"], "log_qz": sites["log_qz"]}
    return fn


def norm_profile(n):
    """d3p_norm_profile through clipping.norm_profile: two calls on one workspace, the counts first, then the quantile positions."""
    def fn(v, rec):
        from d3p_amd import clipping
        norms = (torch.rand(n, generator=torch.Generator().manual_seed(91 + v.seed)) * 3).cuda()
        with _guarded_module(rec, clipping, "norm_profile"):
            prof = clipping.norm_profile(norms, [0.5, 1.0, 2.0], [0.1, 0.5, 0.9])
        flat = []
        for field in prof:     # (a NamedTuple of numbers and tuples of numbers)
            flat.extend(field if isinstance(field, tuple) else (field,))
        return {"profile": torch.tensor([float(x) for x in flat], dtype=torch.float64)}
    return fn


def grad_norms(rows, d):
    """d3p_logreg_grad_norms through clipping.gradient_norms (its workspace comes from DPSVI._workspace)."""
    def fn(v, rec):
        from d3p_amd import clipping
        X, y = _table(rows, d, 95 + v.seed)
        svi = _logreg_svi(d, True, rows)
        st = _logreg_state(svi, d + 1, rows, v, 96)
        norms, losses = clipping.gradient_norms(svi, st, X, y, return_losses=True)
        return {"norms": norms, "losses": losses}
    return fn


SCENARIOS = {}
CALLS = {}       # scenario -> the number of workspaces it takes, one per public call it makes: the refusal test shortens each in turn


def _add(name, fn, calls=1):
    SCENARIOS[name] = fn
    CALLS[name] = calls


for _B, _d, _i in [(16, 4, False), (33, 130, True), (64, 512, False), (20, 512, True), (12, 1500, False), (9, 2600, True)]:
    for _m in (False, True):
        _add(f"logreg-step-B{_B}-d{_d}-{'icpt' if _i else 'plain'}-{'masked' if _m else 'full'}", logreg_step(_B, _d, _i, _m), calls=2)
_add("linreg-step-B50-d96-icpt", logreg_step(50, 96, True, True, family="linear"), calls=2)
_add("poisreg-step-B50-d96-icpt", logreg_step(50, 96, True, False, family="poisson"), calls=2)
_add("logreg-step-K2-B21-d8-icpt", logreg_step(21, 8, True, True, K=2), calls=2)
_add("logreg-step-K2-B21-d513-plain", logreg_step(21, 513, False, False, K=2), calls=2)

_add("logreg-run-d512-B100-12", logreg_run(100, 512, False, 12))
_add("logreg-run-d512-B100-130", logreg_run(100, 512, False, 130))          # a second launch: g0 > 0, the other slot set
_add("logreg-run-d512-icpt-B33-12", logreg_run(33, 512, True, 12))
_add("logreg-run-generic-B64-d300-12", logreg_run(64, 300, False, 12))
_add("logreg-run-generic-B4-d200-icpt-12", logreg_run(4, 200, True, 12))
_add("logreg-run-wide-B64-d2056-12", logreg_run(64, 2056, False, 12))
_add("logreg-run-poisson-B700-d512-icpt-12", logreg_run(700, 512, True, 12, sampler="poisson", N=3000))
_add("logreg-run-sites-B100-d512-12", logreg_run(100, 512, True, 12, guide="sites"))
_add("linreg-run-B64-d96-icpt-12", logreg_run(64, 96, True, 12, family="linear"))
_add("logreg-run-K2-B21-d8-icpt-12", logreg_run(21, 8, True, 12, K=2))
_add("logreg-run-exchange-one-rank-B171-12", logreg_exchange(171, False, 12))

_add("logreg-evaluate-B60-d33", logreg_evaluate(60, 33, False))
_add("logreg-evaluate-K2-B60-d33", logreg_evaluate(60, 33, False, K=2))
_add("logreg-evaluate-sites-B60-d33", logreg_evaluate(60, 33, True, guide="sites"))

_add("gmm-K3-d2-B37", gmm_all(3, 2, 37), calls=5)
_add("gmm-K16-d64-B129", gmm_all(16, 64, 129), calls=5)
_add("gmm-run-K3-d2-B37-70", gmm_run(3, 2, 37, 70))

_add("vae-B5-D12-H7-Z3", vae_all(5, 12, 7, 3, 0), calls=3)
_add("vae-B70-D100-H33-Z9-H21", vae_all(70, 100, 33, 9, 21), calls=3)
_add("vae-B136-D784-H400-Z50-binarised", vae_all(136, 784, 400, 50, 0), calls=3)
_add("vae-B136-D784-H400-Z50-grey", vae_all(136, 784, 400, 50, 0, grey=True), calls=3)

for _N in (105, 4097, 70001):
    _add(f"poisson-select-N{_N}", poisson_select(_N))
_add("poisson-select-batch-N4097-3", poisson_select_batch(4097, 3))
for _P in (1, 257, 20000):
    _add(f"adadp-P{_P}", adadp(_P), calls=2)
_add("predict-vae-B5-n7", predict_vae(5, 7))
_add("vae-log-weights-B5-n45-two-slabs", vae_log_weights(5, 45, 20))
_add("grad-norms-rows70-d33", grad_norms(70, 33))
_add("norm-profile-n1000", norm_profile(1000))


# ---------------------------------------------------------------------------------------------------------------- running them
def _execute(name, fill, v=MAIN, donors=None):
    """One run of a scenario on guarded workspaces: ({output: bytes}, recorder) after (c) was checked."""
    with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)            # (d): the fallback of a stopped run warns
        rec = H.patched(mp, fill, donors=donors)
        out = SCENARIOS[name](v, rec)
        torch.cuda.synchronize()
        got = {k: H.raw_bytes(t) for k, t in out.items()}
        rec.check_all(f"{name} under {fill}")                     # (c)
        assert len(rec.workspaces) == CALLS[name], f"{name}: {len(rec.workspaces)} workspaces went through the harness, {CALLS[name]} declared"
    return got, rec


# (the cases of one scenario are collected next to each other: small caches keep one scenario's reference runs, not all of them)
@functools.lru_cache(maxsize=2)
def _unpatched(name):
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = SCENARIOS[name](MAIN, None)
        torch.cuda.synchronize()
        return {k: H.raw_bytes(t) for k, t in out.items()}


@functools.lru_cache(maxsize=2)
def _zero_run(name):
    return _execute(name, "zero")[0]


@functools.lru_cache(maxsize=1)
def _donor_images(name):
    """The workspaces as the donor run left them, by (purpose, ordinal of the hand-out for that purpose): call i of the run under
    test gets what call i of the donor run left (kept on the host)."""
    _, rec = _execute(name, "zero", v=DONOR)
    return {key: img.cpu() for key, img in rec.images().items()}


def _assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in sorted(want):
        a, b = got[k], want[k]
        assert a.numel() == b.numel(), f"{what}: {k} has {a.numel()} bytes, expected {b.numel()}"
        if not torch.equal(a, b):
            first = int((a != b).nonzero()[0])
            raise AssertionError(f"{what}: output '{k}' differs in {int((a != b).sum())} of {a.numel()} bytes, first at byte {first} "
                                 f"(word {first // 4}): {bytes(a[first // 4 * 4:first // 4 * 4 + 4].tolist()).hex()} != "
                                 f"{bytes(b[first // 4 * 4:first // 4 * 4 + 4].tolist()).hex()}")


@pytest.mark.parametrize("name,fill", [(n, f) for n in sorted(SCENARIOS) for f in H.FILLS])
def test_outputs_do_not_depend_on_what_the_workspace_held(gpu, name, fill):
    if fill == "zero":
        _assert_same(_zero_run(name), _unpatched(name), f"{name}: zero-filled guarded workspaces against the unpatched call")      # (a)
        return
    donors = _donor_images(name) if fill.startswith("replay") else None
    got, rec = _execute(name, fill, donors=donors)
    if fill == "ones":   # the kernels really ran on the buffers of the harness: every workspace handed out was written to
        for g in rec.buffers:
            assert g.nbytes == 0 or bool((g.interior != 0xFF).any()), f"{name}: workspace '{g.tag}' was handed out and never written"
    _assert_same(got, _zero_run(name), f"{name}: workspaces filled with '{fill}' against zero-filled ones")                           # (b)


def test_the_donor_run_differs_from_the_run_under_test(gpu):
    """A donor that left the same bytes behind would make `replay` prove nothing: another key and other data give other outputs and
    another workspace image, at the same sizes."""
    name = "logreg-run-d512-B100-12"
    _, main = _execute(name, "zero")
    img, dimg = main.images(), _donor_images(name)
    assert set(img) == set(dimg) == {("ws", 0)} and img["ws", 0].numel() == dimg["ws", 0].numel()
    assert not torch.equal(img["ws", 0].cpu(), dimg["ws", 0])


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("name,k", [(n, k) for n in sorted(SCENARIOS) for k in range(CALLS[n])])
def test_a_workspace_one_byte_short_is_refused_before_any_launch(gpu, name, k):
    """(e) for EVERY public call of every scenario: the k-th workspace the scenario takes is one byte short (the calls before it run
    as usual, on garbage); call k raises D3PError naming the workspace, and everything it was given is byte-identical to before the
    call -- its workspace and, where the test allocates them, its outputs (interior = the fill, guards intact) and the state it
    started from -- i.e. nothing was launched."""
    import d3p_amd._lib as L
    del _WATCHED[:]
    with pytest.MonkeyPatch.context() as mp:
        rec = H.patched(mp, "bits", short_by=1, short_at=k)
        with pytest.raises(L.D3PError, match="workspace"):
            SCENARIOS[name](MAIN, rec)
        torch.cuda.synchronize()
        assert len(rec.workspaces) == k + 1, f"{name}: the refusal came at workspace {len(rec.workspaces) - 1}, not at {k}"
        short = rec.workspaces[k]
        assert short.nbytes == short.requested - 1
        rec.check_all(f"{name}: after the refusal of call {k}")
        for g in rec.buffers[rec.buffers.index(short):]:          # the refused call's workspace and guarded outputs
            fresh = H.guarded(g.nbytes, g.fill, "cpu", seed=g.seed)
            assert torch.equal(g.interior.cpu(), fresh.interior), f"{name}: '{g.tag}' was written although call {k} was refused"
        for t, before in _WATCHED:
            assert torch.equal(H.raw_bytes(t), H.raw_bytes(before)), f"{name}: the state was written although call {k} was refused"
    del _WATCHED[:]
