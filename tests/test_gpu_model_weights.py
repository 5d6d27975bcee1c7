"""Stacking and Bayesian-bootstrap model weights on the GPU (d3p_stacking_weights, d3p_bb_pseudo_bma, d3p_amd.model_weights) against
tests/model_weights_ref.py, the numpy float64 restatement fed the same float32 matrix and the same threefry bits.

Stacking.  (1) The certificate: the duality gap recomputed on the CPU from the device's w alone is <= tol (1 + 1e-6) when converged, and
|sum w - 1| <= M 2^-52 n_iter.  (2) n_iter is the restatement's and w, gap, f lie within STACK_BOUND of it.  The inputs are chosen so
that n_iter is well-defined: the restatement's gap at the stopping evaluation and at the one before lies outside tol (1 -+ 1e-6), which
every test asserts on the CPU first.  The only difference between the two is float64 rounding order (fused multiply-adds, the strip and
tree order, the device's exp and log), so STACK_BOUND is 16 x the largest deviation MEASURED on the device over this file's cases
(docs/experiments_model_weights.md has the figures): w and gap absolute, f relative.

Bootstrap.  z[b, m] lies within  4 (rows + M + 12) 2^-53 scale_b  of the restatement, scale_b = rows max_m sum_r g |e| / S_b: at most
rows additions per sum plus the product's rounding and the quotient (rows + M + 8 roundings per sum), plus 4 units
for the float64 log (the device's and numpy's are each within 1 ulp, and g enters T and S); T's error and S's each contribute that much
relative to scale_b, on the device and in the restatement: the factor 4.  w lies within 2 max_b bound_z (the softmax's sensitivity) plus
(B + 2 M + 16) 2^-53.  Everything the contract calls independent -- repeated calls, ld, B for a given replicate -- is compared bit for bit.
"""
import numpy as np
import pytest
import torch

from tests import loglik_ref as LR
from tests import model_weights_ref as R
from tests import workspace_harness as WH

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TOL = 1e-6
# 16 x the largest deviation measured on an MI355X over the cases of this file (docs/experiments_model_weights.md)
STACK_BOUND = {"w": 16 * 4.4409e-16, "gap": 16 * 4.4409e-16, "f": 16 * 4.5015e-16}
KEY = np.array([0x9E3779B9, 0x7F4A7C15], np.uint32)
WORST = {"w": 0.0, "gap": 0.0, "f": 0.0, "z": 0.0, "wb": 0.0}


def make(seed, rows, M, variant="plain"):
    rng = np.random.default_rng(seed)
    base = rng.normal(-1.5, 1.0, rows)
    e = base[None, :] + rng.normal(0.0, 0.5, (M, rows)) + np.linspace(0.0, -0.3, M)[:, None]
    if variant == "dominant":
        e[0] += 1.0
    if variant == "duplicate":
        e[M - 1] = e[1]
    return e.astype(np.float32)


@pytest.fixture(scope="module")
def lib(gpu):
    import d3p_amd._lib as L
    return L.load()


def on_device(e, ld=None):
    """The (M, rows) matrix at leading dimension ld on the device; NaN and huge values in the padding."""
    M, rows = e.shape
    ld = rows if ld is None else ld
    buf = torch.full((M, ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, rows::2] = 3.0e38
    buf[:, :rows] = torch.from_numpy(e)
    return buf


def key_on_device(key=KEY):
    return torch.from_numpy(np.asarray(key, np.uint32).view(np.int32).copy()).cuda()


def _stream():
    import d3p_amd._lib as L
    return L.stream_ptr()


def stack(lib, e, ld=None, tol=TOL, max_iter=20000):
    M, rows = e.shape
    buf = on_device(e, ld)
    w = torch.full((M,), 7.0, dtype=torch.float64, device="cuda")
    info = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    need = lib.d3p_stacking_workspace(rows, M)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    rc = lib.d3p_stacking_weights(_stream(), buf.data_ptr(), buf.stride(0), rows, M, tol, max_iter, w.data_ptr(), info.data_ptr(), ws.data_ptr(), need)
    assert rc == 0, lib.d3p_last_error()
    return w.cpu().numpy(), info.cpu().numpy()


def boot(lib, e, B, ld=None, key=KEY):
    M, rows = e.shape
    buf = on_device(e, ld)
    k = key_on_device(key)
    w = torch.full((M,), 7.0, dtype=torch.float64, device="cuda")
    z = torch.full((B, M), 7.0, dtype=torch.float64, device="cuda")
    need = lib.d3p_bb_pseudo_bma_workspace(rows, M, B)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    rc = lib.d3p_bb_pseudo_bma(_stream(), k.data_ptr(), buf.data_ptr(), buf.stride(0), rows, M, B, w.data_ptr(), z.data_ptr(), ws.data_ptr(), need)
    assert rc == 0, lib.d3p_last_error()
    return w.cpu().numpy(), z.cpu().numpy()


def well_defined(gaps, tol):
    """The condition on the inputs that makes n_iter well-defined: the restatement's gap at the stopping evaluation and one before is outside tol (1 -+ 1e-6)."""
    return all(not (tol * (1 - 1e-6) <= g <= tol * (1 + 1e-6)) for g in gaps[-2:])


def check_stack(e, got, tol, max_iter, pair=None, what=""):
    """Conditions 1 and 2 for one run; returns the restatement's result."""
    w, info = got
    M, rows = e.shape
    rw, rj, rconv, rgap, rf, gaps = R.stacking(e, tol, max_iter, history=True)
    assert well_defined(gaps, tol), f"{what}: the input does not define n_iter (gaps {gaps[-2:]})"
    n_iter, conv, gap, f = int(info[0]), bool(info[1]), float(info[2]), float(info[3])
    dev = {"gap": abs(gap - rgap), "f": abs(f - rf) / abs(rf)}
    if pair is None:
        dev["w"] = float(np.abs(w - rw).max())
    else:                                                   # a duplicated column: only the sum of the two weights is determined
        keep = [m for m in range(M) if m not in pair]
        dev["w"] = max(float(np.abs(w[keep] - rw[keep]).max()), abs(w[list(pair)].sum() - rw[list(pair)].sum()))
    print(f"MEASURE stack {what} rows={rows} M={M} n_iter={n_iter}/{rj} conv={conv} dw={dev['w']:.3e} dgap={dev['gap']:.3e} df={dev['f']:.3e}")
    for k, v in dev.items():
        WORST[k] = max(WORST[k], v)
    assert (n_iter, conv) == (rj, rconv), what
    if conv:
        assert R.stacking_gap(e, w) <= tol * (1 + 1e-6), what                         # the certificate, from w alone
        assert gap <= tol
    assert abs(w.sum() - 1.0) <= M * 2.0 ** -52 * max(n_iter, 1), what
    assert (w >= 0).all()
    for k, v in dev.items():
        assert v <= STACK_BOUND[k], (what, k, v)
    return rw, rj, rconv, rgap, rf


def check_boot(e, got, B, what="", b0=0):
    w, z = got
    M, rows = e.shape
    rw, rz, scale = R.bb_pseudo_bma(KEY, e, B, b0)
    bound_z = 4 * (rows + M + 12) * U * scale
    fin = np.isfinite(rz)
    assert (z[~fin] == rz[~fin]).all(), what                                          # -inf where the restatement has -inf
    err = np.where(fin, np.abs(z - np.where(fin, rz, 0.0)), 0.0)
    ratio_z = float((err / bound_z[:, None]).max())
    if b0 == 0:
        bound_w = 2 * float(bound_z.max()) + (B + 2 * M + 16) * U
        ratio_w = float(np.abs(w - rw).max() / bound_w)
    else:
        ratio_w = 0.0
    print(f"MEASURE boot {what} rows={rows} M={M} B={B} err/bound z={ratio_z:.4f} w={ratio_w:.4f}")
    WORST["z"], WORST["wb"] = max(WORST["z"], ratio_z), max(WORST["wb"], ratio_w)
    assert ratio_z <= 1.0 and ratio_w <= 1.0, what
    if b0 == 0:
        assert abs(w.sum() - 1.0) <= (B + 2 * M + 16) * U
    return rw, rz


# ------------------------------------------------------------------------------------------------ agreement and certificate
CASES = [(131372, 3, "dominant", 1), (257, 3, "plain", 6), (1000, 4, "plain", 3), (2049, 5, "dominant", 4), (4099, 16, "plain", 4), (10000, 7, "duplicate", 3),
         (513, 16, "plain", 5), (777, 2, "plain", 5)]


@pytest.mark.parametrize("rows,M,variant,seed", CASES)
def test_stacking_agrees_with_the_restatement_and_holds_its_certificate(lib, rows, M, variant, seed):
    e = make(seed, rows, M, variant)
    pair = (1, M - 1) if variant == "duplicate" else None
    rw, rj, rconv, _, _ = check_stack(e, stack(lib, e, ld=rows + 5), TOL, 20000, pair, f"{variant}/{seed}")
    assert rconv and 15 <= rj <= 2100                                              # (rows = 131372: two chunks per strip)
    if variant == "dominant":
        assert rw[0] > 1 - 1e-5


EDGE_ROWS = (1, 63, 64, 65, 255, 256, 257, 513)          # L = 256 rows per strip and per staged chunk: L - 1, L, L + 1, 2 L + 1


@pytest.mark.parametrize("M,B", [(1, 1), (2, 63), (3, 64), (16, 65)])
@pytest.mark.parametrize("rows", EDGE_ROWS)
def test_edge_shapes_with_padding(lib, rows, M, B):
    assert lib.d3p_stacking_strip_rows() == lib.d3p_bb_pseudo_bma_strip_rows() == 256
    e = make(100 + rows + M, rows, M)
    tol, most = 1e-5, 300
    got = stack(lib, e, ld=rows + 3, tol=tol, max_iter=most)
    check_stack(e, got, tol, most, None, f"edge")
    tight = stack(lib, e, ld=rows, tol=tol, max_iter=most)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, tight))                # ld changes nothing
    bgot = boot(lib, e, B, ld=rows + 3)
    check_boot(e, bgot, B, "edge")
    btight = boot(lib, e, B, ld=rows)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(bgot, btight))
    if M == 1:
        assert got[0].tolist() == [1.0] and got[1][:3].tolist() == [0.0, 1.0, 0.0] and bgot[0].tolist() == [1.0]


def test_identical_models_keep_equal_weights(lib):
    one = make(3, 300, 1)[0]
    w, info = stack(lib, np.stack([one, one, one, one]))
    assert w.tolist() == [0.25] * 4 and info[:3].tolist() == [0.0, 1.0, 0.0]
    wb, z = boot(lib, np.stack([one, one]), 10)
    assert wb.tolist() == [0.5, 0.5] and (z[:, 0] == z[:, 1]).all()


# ------------------------------------------------------------------------------------------------ early exit and cut-off
def test_cut_off_and_host_chunk_sizes(lib):
    rows, M, variant, seed = CASES[2]
    e = make(seed, rows, M, variant)
    full = stack(lib, e)
    need = int(full[1][0])
    assert bool(full[1][1]) and need > 100
    # a max_iter below the needed count: not converged, n_iter = max_iter, the restatement's w at that count
    for most in (1, 64, need - 7):
        got = stack(lib, e, max_iter=most)
        rw, rj, rconv, _, _ = check_stack(e, got, TOL, most, None, f"cut-off {most}")
        assert (int(got[1][0]), bool(got[1][1])) == (most, False) and rj == most and not rconv
    # max_iter exactly the needed count converges at it
    got = stack(lib, e, max_iter=need)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, full))
    # the host's chunk size changes nothing: the launches behind the stopping one write nothing
    before = lib.d3p_stacking_set_chunk(0)
    try:
        for chunk in (64, 100, need + 1, 4096):                                        # (the last two: larger than n_iter)
            assert lib.d3p_stacking_set_chunk(chunk) >= 64
            got = stack(lib, e)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, full)), chunk
        cut = {}
        for chunk in (64, 65, 4096):
            lib.d3p_stacking_set_chunk(chunk)
            cut[chunk] = stack(lib, e, max_iter=64)                                    # evaluation 64 is the 65th: a chunk's first / last
        assert all(a.tobytes() == b.tobytes() for c in (65, 4096) for a, b in zip(cut[c], cut[64]))
    finally:
        lib.d3p_stacking_set_chunk(before)


# ------------------------------------------------------------------------------------------------ bootstrap
def test_bootstrap_replicates_bits_and_statistics(lib):
    rows, M = 97, 3
    e = make(11, rows, M)
    w1000, z1000 = boot(lib, e, 1000)
    check_boot(e, (w1000, z1000), 1000, "B=1000")
    again = boot(lib, e, 1000, ld=rows + 31)
    assert again[0].tobytes() == w1000.tobytes() and again[1].tobytes() == z1000.tobytes()      # repeated call, another ld
    w65, z65 = boot(lib, e, 65)
    assert z65.tobytes() == z1000[:65].tobytes()                                      # replicate b alone or among others
    _, z1 = boot(lib, e, 1)
    assert z1.tobytes() == z1000[:1].tobytes()
    other = boot(lib, e, 65, key=np.array([1, 2], np.uint32))[1]
    assert not (other == z65).any()
    # statistically sane: the replicates' means lie within 5 bootstrap standard errors of rows * mean_r e
    total = e.astype(np.float64).sum(axis=1)
    assert (np.abs(z1000.mean(axis=0) - total) <= 5 * z1000.std(axis=0) / np.sqrt(1000)).all()
    assert (z1000.std(axis=0) > 0).all() and abs(w1000.sum() - 1) < 1e-12 and (w1000 > 0).all()


def test_bootstrap_over_several_strips_and_blocks(lib):
    """More chunks than one strip holds (129 chunks: per = 2) and more replicates than one workgroup (B = 300)."""
    rows, M, B = 128 * 256 + 77, 5, 300
    e = make(12, rows, M)
    got = boot(lib, e, B)
    check_boot(e, got, B, "strips")
    got4 = boot(lib, e[:4], 70, ld=rows)
    check_boot(e[:4], got4, 70, "strips, MT = 4")


# ------------------------------------------------------------------------------------------------ special values
@pytest.mark.parametrize("rows", (65, 513))
def test_special_values(lib, rows):
    M, B = 5, 65
    e = make(20 + rows, rows, M)
    some = e.copy()
    some[4, 0] = some[2, rows - 1] = some[4, rows // 2] = -np.inf                     # legitimate: p = 0 there; pseudo-BMA gives no weight
    got = stack(lib, some, ld=rows + 1)
    check_stack(some, got, TOL, 20000, None, "-inf")
    bgot = boot(lib, some, B)
    _, rz = check_boot(some, bgot, B, "-inf")
    assert (bgot[1][:, [2, 4]] == -np.inf).all() and np.isfinite(bgot[1][:, [0, 1, 3]]).all() and bgot[0][2] == 0.0
    for name, m, r, v in (("nan first", 0, 0, np.nan), ("nan last", M - 1, rows - 1, np.nan), ("+inf", 1, rows // 3, np.inf),
                          ("all -inf", None, rows - 2, -np.inf)):
        bad = e.copy()
        if m is None:
            bad[:, r] = v
        else:
            bad[m, r] = v
        w, info = stack(lib, bad)
        assert np.isnan(w).all() and np.isnan(info[2:]).all() and info[1] == 0.0, name
        assert np.isnan(R.stacking(bad)[0]).all()
        wb, z = boot(lib, bad, B)
        assert np.isnan(wb).all() and np.isnan(z).all(), name


# ------------------------------------------------------------------------------------------------ workspaces
def _guarded_call(lib, kind, buf, rows, M, B, fill, donor=None, short=0):
    need = lib.d3p_stacking_workspace(rows, M) if kind == "stack" else lib.d3p_bb_pseudo_bma_workspace(rows, M, B)
    ws = WH.guarded(need - short, fill, "cuda", donor=donor)
    a = WH.guarded(8 * M, "bits", "cuda", seed=1)
    b = WH.guarded(32 if kind == "stack" else 8 * B * M, "bits", "cuda", seed=2)
    before = [WH.raw_bytes(g.interior) for g in (a, b, ws)]
    if kind == "stack":
        rc = lib.d3p_stacking_weights(_stream(), buf.data_ptr(), buf.stride(0), rows, M, TOL, 20000, a.interior.data_ptr(), b.interior.data_ptr(),
                                      ws.interior.data_ptr(), need - short)
    else:
        k = key_on_device()
        rc = lib.d3p_bb_pseudo_bma(_stream(), k.data_ptr(), buf.data_ptr(), buf.stride(0), rows, M, B, a.interior.data_ptr(), b.interior.data_ptr(),
                                   ws.interior.data_ptr(), need - short)
    torch.cuda.synchronize()
    for g in (a, b, ws):
        g.check(f"{kind} / {fill}")
    return rc, a, b, ws, before


@pytest.mark.parametrize("kind", ("stack", "boot"))
def test_workspaces_under_every_fill(lib, kind):
    rows, M, B = 257 * 3, 5, 70
    buf = on_device(make(31, rows, M), rows + 9)
    rc, a0, b0, ws0, _ = _guarded_call(lib, kind, buf, rows, M, B, "zero")
    assert rc == 0
    want = [WH.raw_bytes(a0.interior), WH.raw_bytes(b0.interior)]
    donor = ws0.image()
    for fill in WH.FILLS:
        rc, a, b, ws, _ = _guarded_call(lib, kind, buf, rows, M, B, fill, donor=donor)
        assert rc == 0, fill
        assert torch.equal(WH.raw_bytes(a.interior), want[0]) and torch.equal(WH.raw_bytes(b.interior), want[1]), fill
    # one byte short: refused with nothing written
    rc, a, b, ws, before = _guarded_call(lib, kind, buf, rows, M, B, "bits", short=1)
    assert rc == -4 and b"workspace too small" in lib.d3p_last_error()
    assert all(torch.equal(WH.raw_bytes(g.interior), was) for g, was in zip((a, b, ws), before))


# ------------------------------------------------------------------------------------------------ end to end
def test_compare_models_end_to_end(gpu):
    from d3p_amd import criteria as CR
    from d3p_amd import model_weights as MW
    from d3p_amd.models import LinearRegression, PoissonRegression
    n, rows, d = 64, 2000, 4
    X, y, W, b = LR.inputs("poisson", n, rows, d, True)
    Xt, yt = torch.tensor(X).cuda(), torch.tensor(y).cuda()
    s = {"w": torch.tensor(np.array(W)).cuda(), "intercept": torch.tensor(np.array(b)).cuda()}
    results = {"poisson": CR.loo(PoissonRegression(d, intercept=True), s, Xt, yt, pointwise=True),
               "linear": CR.loo(LinearRegression(d, intercept=True, obs_scale=LR.SIGMA["linear"]), s, Xt, yt, pointwise=True),
               "poisson0": CR.loo(PoissonRegression(d, intercept=False), {"w": s["w"]}, Xt, yt, pointwise=True)}
    table = MW.compare_models(results, tol=1e-6)
    mw = MW.stacking_weights(results, tol=1e-6)
    assert mw.names == ("poisson", "linear", "poisson0") and mw.method == "stacking" and mw.converged and mw.n_iter >= 0
    assert mw.weights.is_cuda and mw.weights.dtype == torch.float64 and mw.gap.is_cuda and mw.stacked_elpd.is_cuda
    assert table.weights.weights.cpu().numpy().tobytes() == mw.weights.cpu().numpy().tobytes()
    elpd = {k: float(r.elpd_loo) for k, r in results.items()}
    assert list(table.names) == sorted(elpd, key=lambda k: -elpd[k]) and table.rank == (0, 1, 2) and table.kind == "loo"
    best = results[table.names[0]]
    for i, name in enumerate(table.names):
        want = CR.compare(best, results[name])
        assert float(table.elpd_diff[i]) == float(want.elpd_diff) and float(table.dse[i]) == float(want.se_diff)
        assert float(table.elpd[i]) == elpd[name] and float(table.se[i]) == float(results[name].se)
        assert float(table.p[i]) == float(results[name].p_loo)
        assert float(table.weight[i]) == float(mw.weights[mw.names.index(name)])
        assert table.warning[i] == (int(results[name].n_high_k) > 0)
    assert float(table.elpd_diff[0]) == 0.0 and float(table.dse[0]) == 0.0 and "elpd_loo" in table.table()
    e = np.stack([r.pointwise["elpd_loo"].cpu().numpy() for r in results.values()])
    if np.isfinite(e).all():
        rw, rj, rconv, rgap, rf = R.stacking(e, 1e-6, 20000)
        assert rconv == mw.converged and np.abs(mw.weights.cpu().numpy() - rw).max() <= 1e-6
        assert R.stacking_gap(e, mw.weights.cpu().numpy()) <= 1e-6 * (1 + 1e-6)
    # pseudo-BMA and pseudo-BMA+ on the same results
    plain = MW.pseudo_bma_weights(results)
    tot = np.array([elpd[k] for k in plain.names])
    ex = np.exp(tot - tot.max())
    assert plain.method == "pseudo-BMA" and np.abs(plain.weights.cpu().numpy() - ex / ex.sum()).max() <= 1e-12
    plus = MW.pseudo_bma_weights(results, rng_key=key_on_device(), n_boot=200)
    assert plus.method == "pseudo-BMA+" and plus.se_boot.shape == (3,) and abs(float(plus.weights.sum()) - 1) < 1e-12
    if np.isfinite(e).all():
        rw, rz, _ = R.bb_pseudo_bma(KEY, e, 200)
        assert np.abs(plus.weights.cpu().numpy() - rw).max() <= 1e-9 and np.abs(plus.se_boot.cpu().numpy() / rz.std(axis=0) - 1).max() <= 1e-9
    t2 = MW.compare_models(results, method="pseudo-BMA+", rng_key=key_on_device(), n_boot=200)
    assert t2.weights.weights.cpu().numpy().tobytes() == plus.weights.cpu().numpy().tobytes() and t2.names == table.names
    waic = {k: CR.waic(m, ss, Xt, yt, pointwise=True) for k, (m, ss) in
            {"poisson": (PoissonRegression(d, intercept=True), s), "poisson0": (PoissonRegression(d, intercept=False), {"w": s["w"]})}.items()}
    tw = MW.compare_models(waic)
    assert tw.kind == "waic" and tw.warning == (False, False) and abs(float(tw.weight.sum()) - 1) < 1e-9


def test_public_functions_run_on_guarded_memory(gpu, monkeypatch):
    """The module's own allocations (workspace and outputs) replaced by guarded, garbage-filled ones: same bits, guards intact."""
    from d3p_amd import model_weights as MW
    e = on_device(make(41, 700, 6), 701)[:, :700]
    want_s = [t.cpu().numpy().tobytes() for t in MW.stacking_from_matrix(e, tol=1e-5)]
    want_b = [t.cpu().numpy().tobytes() for t in MW.bootstrap_from_matrix(key_on_device(), e, n_boot=40)]
    for fill in ("ones", "big", "bits"):
        rec = WH.Recorder(fill, 0, None)
        WH.guarded_empty(monkeypatch, MW, rec, "model_weights")
        got_s = [t.cpu().numpy().tobytes() for t in MW.stacking_from_matrix(e, tol=1e-5)]
        got_b = [t.cpu().numpy().tobytes() for t in MW.bootstrap_from_matrix(key_on_device(), e, n_boot=40)]
        torch.cuda.synchronize()
        rec.check_all(fill)
        monkeypatch.undo()
        assert got_s == want_s and got_b == want_b and len(rec.workspaces) == 2, fill


def test_example_prints_the_comparison_table(gpu, capsys):
    """examples/poisson_regression.py --compare-models on a small table: four fits, the table with stacking weights, pseudo-BMA+."""
    import argparse
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "poisson_regression.py")
    spec = importlib.util.spec_from_file_location("poisson_regression_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(argparse.Namespace(sigma=0.5, clip_threshold=1.0, num_steps=300, learning_rate=2e-2, batch_size=200, dimensions=4,
                                num_samples=2000, compare_models=32))
    lines = capsys.readouterr().out.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("model comparison (2000 rows, 32 posterior draws each)")]
    assert len(at) == 1
    head, rows = lines[at[0] + 1], [l.split() for l in lines[at[0] + 2:at[0] + 6]]
    assert head.split() == ["model", "rank", "elpd_loo", "p_loo", "elpd_diff", "dse", "weight", "se", "warning"]
    assert sorted(r[0] for r in rows) == ["linear", "linear+1", "poisson", "poisson+1"] and [r[1] for r in rows] == ["0", "1", "2", "3"]
    elpd = [float(r[2]) for r in rows]
    assert elpd == sorted(elpd, reverse=True) and float(rows[0][4]) == 0.0 and float(rows[0][5]) == 0.0
    assert abs(sum(float(r[6]) for r in rows) - 1.0) <= 4 * 0.0005 + 1e-9            # (four weights printed to three decimals)
    assert rows[0][0].startswith("poisson")                                          # counts: a Poisson model leads
    assert lines[at[0] + 6].startswith("stacking: ") and "duality gap" in lines[at[0] + 6]
    assert lines[at[0] + 7].startswith("pseudo-BMA+ (1000 bootstrap replicates): ") and lines[at[0] + 7].count("se_boot") == 4


def test_zz_report_worst(lib):
    """Prints the largest deviations this file measured (the figures of docs/experiments_model_weights.md); asserts nothing new."""
    print("MEASURE worst " + " ".join(f"{k}={v:.4e}" for k, v in WORST.items()))
