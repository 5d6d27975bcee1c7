"""d3p_amd.ppc on the GPU: d3p_rep_stats against the CPU restatement (tests/ppc_ref.py) at every edge of its tiling and for the special
values; d3p_predict_stats against d3p_rep_stats of the matrix the sampling entries store; the Python layer against the *_samples
calls; two deterministic checks of what posterior_predictive_check means; the workspace contract; the C refusals.  Every comparison
is BY VALUE (NaN equal to NaN), never within a tolerance."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from d3p_amd import _lib as L
from d3p_amd import ppc
from d3p_amd import predictive as Ps
from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, LinearRegression, LogisticRegression, MeanFieldGuide,
                            PoissonRegression)

from . import ppc_ref as R
from . import workspace_harness as H
from .predictive_ref import key, logreg_params, np_

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
FAMILIES = {"linear": L.D3P_FAMILY_LINREG, "poisson": L.D3P_FAMILY_POISSON, "logistic": L.D3P_FAMILY_LOGREG}
SIGMA = 0.75


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _rep_stats_c(m, ld, n, rows, shift=0.0):
    """d3p_rep_stats on a device tensor whose draw s starts at element s * ld: (5, n) float64 as numpy."""
    lib = L.load()
    out = torch.empty((5, n), dtype=torch.float64, device=DEV)
    nbytes = lib.d3p_rep_stats_workspace(rows, n)
    assert nbytes == R.strips(rows)[2] * 5 * n * 8
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    L.check(lib.d3p_rep_stats(L.stream_ptr(), L.ptr(m), 0 if m.dtype == torch.float32 else 1, ld, n, rows, shift, L.ptr(out), L.ptr(ws), nbytes))
    return np_(out)


def _random_matrix(dtype, n, rows, seed):
    rng = np.random.default_rng(seed)
    if dtype == "float32":
        return (rng.normal(size=(n, rows)) * 10 ** rng.uniform(-1, 2, size=(n, 1))).astype(np.float32)
    m = rng.poisson(3.0, size=(n, rows)).astype(np.int32)
    m[rng.random(size=(n, rows)) < 0.1] = -7
    return m


# ------------------------------------------------------------------------------- d3p_rep_stats against the restatement
@pytest.mark.parametrize("dtype", ["float32", "int32"])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 127, 128, 129, 257])
def test_rep_stats_rows_at_every_tile_edge(gpu, dtype, rows):
    n = 5
    m = _random_matrix(dtype, n, rows, 100 + rows)
    for shift in (0.0, 2.625):
        got = _rep_stats_c(_dev(m), rows, n, rows, shift)
        assert R.same(got, R.rep_stats(m, shift)), (dtype, rows, shift)


@pytest.mark.parametrize("dtype", ["float32", "int32"])
@pytest.mark.parametrize("rows", [65536, 65537])
def test_rep_stats_strips_of_one_and_two_tiles(gpu, dtype, rows):
    """65 536 rows: 512 strips of one tile; 65 537: the only shape class with per = 2 (257 strips, the last of one tile and one row)."""
    n = 3
    m = _random_matrix(dtype, n, rows, rows)
    shift = float(np.float32(m.mean()))
    got = _rep_stats_c(_dev(m), rows, n, rows, shift)
    assert R.same(got, R.rep_stats(m, shift))


@pytest.mark.parametrize("dtype", ["float32", "int32"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 128, 129])
def test_rep_stats_draws_at_every_tile_edge_with_a_padded_ld(gpu, dtype, n):
    rows, ld = 161, 173
    m = _random_matrix(dtype, n, rows, 7 * n)
    buf = np.full((n, ld), 12345, m.dtype)             # what lies between the rows' ends must not be read
    buf[:, :rows] = m
    ref = R.rep_stats(m, -1.5)
    assert R.same(_rep_stats_c(_dev(buf), ld, n, rows, -1.5), ref)
    assert R.same(_rep_stats_c(_dev(m), rows, n, rows, -1.5), ref)          # a draw's result does not depend on ld
    if n > 1:                                                                # ... nor on n or on the other draws
        one = _rep_stats_c(_dev(buf)[n - 1:], ld, 1, rows, -1.5)
        assert R.same(one[:, 0], ref[:, n - 1])


def test_rep_stats_special_values(gpu):
    rows = 200
    rng = np.random.default_rng(3)
    m = rng.normal(size=(6, rows)).astype(np.float32)
    m[0, [0, 40, 199]] = [0.0, -0.0, 0.0]
    m[1, 130] = np.inf
    m[2, [5, 150]] = [-np.inf, np.inf]
    m[3, 77] = np.nan                                   # one draw only
    m[4, :] = 3.25                                      # a constant column of the rows x draws picture
    clean = m.copy()
    clean[3, 77] = 0.5
    got, ref = _rep_stats_c(_dev(m), rows, 6, rows, 0.25), R.rep_stats(m, 0.25)
    assert R.same(got, ref)
    assert np.isnan(got[:4, 3]).all() and got[4, 3] == 0 and got[4, 0] == 3
    assert got[0, 1] == np.inf and got[3, 1] == np.inf and np.isnan(got[0, 2]) and got[2, 2] == -np.inf and got[3, 2] == np.inf
    assert got[:, 4].tolist() == [rows * 3.0, rows * 9.0, 3.25, 3.25, 0.0]
    other = _rep_stats_c(_dev(clean), rows, 6, rows, 0.25)
    keep = [0, 1, 2, 4, 5]
    assert np.array_equal(got[:, keep].view(np.uint64), other[:, keep].view(np.uint64))      # the NaN leaves the other draws' BITS alone
    mi = rng.integers(-5, 5, size=(3, rows)).astype(np.int32)
    mi[0, [3, 190]] = [INT_MIN, INT_MAX]
    mi[1, :] = 0
    mi[2, 64] = INT_MAX
    got = _rep_stats_c(_dev(mi), rows, 3, rows, 0.0)
    assert R.same(got, R.rep_stats(mi, 0.0))
    assert got[2, 0] == INT_MIN and got[3, 0] == INT_MAX and got[3, 2] == INT_MAX and got[:, 1].tolist() == [0.0, 0.0, 0.0, 0.0, float(rows)]


def test_rep_stats_two_calls_give_identical_bits(gpu):
    m = _random_matrix("float32", 130, 1000, 9)
    md = _dev(m)
    a, b = _rep_stats_c(md, 1000, 130, 1000, 0.1), _rep_stats_c(md, 1000, 130, 1000, 0.1)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert R.same(a, R.rep_stats(m, 0.1))


# ------------------------------------------------------------------------------- the fused form against the stored matrix
def _problem(family, d, rows, n, intercept, seed):
    """X, the latent buffer (n, ld) with the weights at w_off and the intercept at b_col, random obs keys.  Poisson: predictors spread
    over both branches of the rule, a NaN row (marker -1) and an overflowing rate in draw 0 (marker INT_MAX)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, size=(rows, d)).astype(np.float32)
    ld, w_off, b_col = d + 3, 2, (0 if intercept else -1)
    lat = rng.normal(size=(n, ld)).astype(np.float32)
    lat[:, w_off:w_off + d] *= np.float32(4.0 / np.sqrt(d))
    if intercept:
        lat[:, b_col] = rng.uniform(-1, 2, size=n).astype(np.float32)
    if family == "poisson" and rows >= 3:
        X[0, :] = np.nan
        X[1, :] = 0.0
        X[1, 0] = 200.0
        lat[0, w_off] = 1.0
    keys = rng.integers(0, 2 ** 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
    return X, lat, ld, w_off, b_col, keys


def _model_struct(family, d, intercept):
    return L.LogregModel(d, int(intercept), 1.0, 1.0, 1.0, 1.0, FAMILIES[family], L.D3P_GUIDE_SOFTPLUS, SIGMA if family == "linear" else 0.0)


def _stored(family, Xd, latd, ld, w_off, b_col, kd, d, rows, n, intercept):
    lib = L.load()
    obs = torch.empty((n, rows), dtype=torch.float32 if family == "linear" else torch.int32, device=DEV)
    if family == "logistic":
        L.check(lib.d3p_predict_logreg(L.stream_ptr(), L.ptr(Xd), rows, d, L.ptr(latd), ld, w_off, b_col, n, L.ptr(kd), L.ptr(obs)))
    else:
        ms = _model_struct(family, d, intercept)
        L.check(lib.d3p_predict_glm(L.stream_ptr(), C.byref(ms), L.ptr(Xd), rows, d, L.ptr(latd), ld, w_off, b_col, n, L.ptr(kd), L.ptr(obs)))
    return obs


def _fused(family, Xd, latd, ld, w_off, b_col, kd, d, rows, n, intercept, shift):
    lib = L.load()
    out = torch.empty((5, n), dtype=torch.float64, device=DEV)
    nbytes = lib.d3p_rep_stats_workspace(rows, n)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    ms = _model_struct(family, d, intercept)
    L.check(lib.d3p_predict_stats(L.stream_ptr(), C.byref(ms), L.ptr(Xd), rows, d, L.ptr(latd), ld, w_off, b_col, n, L.ptr(kd), shift,
                                  L.ptr(out), L.ptr(ws), nbytes))
    return np_(out)


# d on both sides of a K slice, rows and draws on both sides of a tile, with and without an intercept; the last reaches per = 2
FUSED_CASES = [(1, 1, 1, False), (32, 33, 33, False), (33, 128, 129, True), (1, 129, 33, True), (32, 300, 129, False), (33, 300, 1, False),
               (33, 129, 33, False), (1, 65537, 3, False)]


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("d,rows,n,intercept", FUSED_CASES)
def test_predict_stats_equals_rep_stats_of_the_stored_matrix(gpu, family, d, rows, n, intercept):
    X, lat, ld, w_off, b_col, keys = _problem(family, d, rows, n, intercept, 31 * d + 7 * rows + n)
    Xd, latd, kd = _dev(X), _dev(lat), _dev(keys)
    obs = _stored(family, Xd, latd, ld, w_off, b_col, kd, d, rows, n, intercept)
    shift = 0.0 if rows == 1 else 1.375
    want = _rep_stats_c(obs, rows, n, rows, shift)
    got = _fused(family, Xd, latd, ld, w_off, b_col, kd, d, rows, n, intercept, shift)
    assert R.same(got, want), (family, d, rows, n, intercept)
    assert np.array_equal(got[:2].view(np.uint64), want[:2].view(np.uint64))          # the sums: bit for bit
    assert R.same(want, R.rep_stats(np_(obs), shift))                                  # ... and both are the restatement's
    again = _fused(family, Xd, latd, ld, w_off, b_col, kd, d, rows, n, intercept, shift)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    if family == "poisson" and rows >= 3:
        o = np_(obs)
        assert (got[2] == -1).all() and (o[:, 0] == -1).all()                          # the NaN row's marker, in every draw
        assert got[3, 0] == INT_MAX and o[0, 1] == INT_MAX                             # the overflowing rate's, in draw 0
        if rows >= 33:
            t = lat[:, w_off:w_off + d].astype(np.float64) @ X[2:].astype(np.float64).T + (lat[:, b_col:b_col + 1] if intercept else 0.0)
            assert (t < 2.0).any() and (t > 2.6).any()                            # inversion (rate < 10) and rejection both occur
    if family == "logistic" and rows * n >= 64:
        assert 0 < got[4].sum() < rows * n and got[2].min() == 0 and got[3].max() == 1


# ------------------------------------------------------------------------------- the Python layer
def _family_model(family, d, intercept):
    if family == "linear":
        return LinearRegression(d, intercept=intercept, obs_scale=SIGMA)
    return PoissonRegression(d, intercept=intercept) if family == "poisson" else LogisticRegression(d, intercept=intercept)


def _assert_stats_equal(a, b):
    assert a.n_rows == b.n_rows and a.shift == b.shift
    for x, y in zip(a._five(), b._five()):
        assert x.dtype == torch.float64 and x.is_cuda and x.shape == y.shape
        assert R.same(np_(x), np_(y))


def _guide_cases():
    out = [(f, g) for f in FAMILIES for g in (AutoDiagonalNormal, DiagonalNormalGuide)]
    return out + [("logistic", MeanFieldGuide)]


def _guide_params(guide, d, rng):
    p = logreg_params(guide, d, True, rng)
    for name in p:                                       # predictors of moderate size: every family's outcomes vary
        if name.endswith("_loc"):
            p[name] = (np.asarray(p[name]) * 0.3).astype(np.float32)
    return p


@pytest.mark.parametrize("family,guide_cls", _guide_cases())
def test_python_layer_equals_replicate_stats_of_the_samples(gpu, family, guide_cls):
    rng = np.random.default_rng(41)
    d, rows, n = 5, 300, 33
    X = rng.uniform(-1, 1, size=(rows, d)).astype(np.float32)
    model = _family_model(family, d, True)
    guide = guide_cls(model)
    params = _guide_params(guide, d, rng)
    k, shift = key(77), 0.75
    res = Ps.posterior_predictive_samples(k, n, model, (X,), guide, params)
    latents, stats = ppc.posterior_predictive_stats(k, n, model, (X,), guide, params, shift=shift)
    assert set(latents) == {"w", "intercept"}
    assert torch.equal(latents["w"], res["w"]) and torch.equal(latents["intercept"].reshape(n), res["intercept"].reshape(n))   # bit for bit
    _assert_stats_equal(stats, ppc.replicate_stats(res["obs"], shift))
    assert tuple(stats.sum.shape) == (n,) and stats.n_rows == rows
    # given samples: predictive_samples' key rule
    K = key(78)
    obs = Ps.predictive_samples(K, model, res, X)
    _assert_stats_equal(ppc.predictive_stats(K, model, res, X, shift=shift), ppc.replicate_stats(obs, shift))
    one = {"w": res["w"][2], "intercept": res["intercept"].reshape(n)[2]}
    single = ppc.predictive_stats(K, model, one, X)
    assert tuple(single.sum.shape) == () and single.shift == 0.0
    _assert_stats_equal(single, ppc.replicate_stats(Ps.predictive_samples(K, model, one, X)))
    # the derived statistics are float64 functions of the five
    ref = R.rep_stats(np_(res["obs"]), shift)
    assert np.array_equal(np_(stats.mean), shift + ref[0] / rows)
    assert np.array_equal(np_(stats.var()), (ref[1] - ref[0] * ref[0] / rows) / (rows - 1))
    assert np.array_equal(np_(stats.zero_share), ref[4] / rows)


def test_replicate_stats_reads_views_in_place_and_copies_what_it_must(gpu):
    m = _random_matrix("int32", 6, 150, 2)
    md = _dev(m)
    ref = R.rep_stats(m, 1.0)
    _assert_np = lambda st, want: all(R.same(np_(x).reshape(-1), w) for x, w in zip(st._five(), want))
    assert _assert_np(ppc.replicate_stats(md, 1.0), ref)
    assert _assert_np(ppc.replicate_stats(md[1:5, 10:140], 1.0), R.rep_stats(m[1:5, 10:140], 1.0))       # ld > rows, in place
    assert _assert_np(ppc.replicate_stats(md.t().contiguous().t(), 1.0), ref)                              # last stride != 1: copied
    assert _assert_np(ppc.replicate_stats(md[0].reshape(1, -1).expand(4, 150), 1.0), R.rep_stats(np.repeat(m[:1], 4, 0), 1.0))
    one = ppc.replicate_stats(md[3])
    assert tuple(one.min.shape) == () and _assert_np(one, R.rep_stats(m[3], 0.0)[:, 0].reshape(5, 1))


# ------------------------------------------------------------------------------- what posterior_predictive_check means
@pytest.mark.parametrize("family", list(FAMILIES))
def test_check_of_a_replicated_row_against_itself(gpu, family):
    """(a) y = draw 0's own replicated row: T(y) is T(y_rep_0) for every statistic, so both tail shares are at least 1 / n."""
    rng = np.random.default_rng(5)
    d, rows, n = 4, 257, 20
    X = rng.uniform(-1, 1, size=(rows, d)).astype(np.float32)
    model = _family_model(family, d, True)
    guide = AutoDiagonalNormal(model)
    params = _guide_params(guide, d, rng)
    k = key(3)
    y = Ps.posterior_predictive_samples(k, n, model, (X,), guide, params)["obs"][0]
    res = ppc.posterior_predictive_check(k, n, model, (X, y.to(torch.float32)), guide, params, statistics=ppc.STATISTICS)
    assert res.statistic == ppc.STATISTICS and res.n_draws == n and res.n_rows == rows and res.n_marked == 0
    for name in ppc.STATISTICS:
        rep = res.replicated[name]
        assert rep.shape == (n,) and rep.dtype == np.float64
        assert R.same(res.observed[name], rep[0]), name
        if not np.isnan(rep[0]):
            assert res.p_ge[name] >= 1 / n and res.p_le[name] >= 1 / n
        assert res.p_ge[name] == (rep >= res.observed[name]).sum() / n and res.p_le[name] == (rep <= res.observed[name]).sum() / n
    assert len(res.lines()) == len(ppc.STATISTICS)


def test_check_finds_zero_inflation_in_a_poisson_fit(gpu):
    """(b) 2000 rows at a predictor near 2 (rate 7.4), latents one weight vector with 1e-3 jitter, half of y overwritten with 0: a
    replicated data set holds about 2000 exp(-7.4) = 1.2 zeros against at least 1000 observed, and its dispersion stays near 1
    (margins for any key: tests/test_ppc_host.py, test_poisson_check_margin_on_the_cpu)."""
    rng = np.random.default_rng(8)
    d, rows, n = 4, 2000, 50
    X = rng.uniform(-1, 1, size=(rows, d)).astype(np.float32)
    model = PoissonRegression(d, intercept=True)
    guide = AutoDiagonalNormal(model)
    params = {"auto_loc": np.array([0.01, -0.01, 0.02, 0.0, 2.0], np.float32), "auto_scale": np.full(5, 1e-3, np.float32)}
    y = Ps.posterior_predictive_samples(key(1), 1, model, (X,), guide, params)["obs"][0].clone()
    y[::2] = 0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = ppc.posterior_predictive_check(key(2), n, model, (X, y), guide, params, statistics=("zeros", "dispersion", "mean"))
    assert not [w for w in caught if "Poisson marker" in str(w.message)]                 # no marker, no warning
    assert res.observed["zeros"] >= 1000 and res.replicated["zeros"].max() <= 12
    assert res.p_ge["zeros"] == 0.0 and res.p_le["zeros"] == 1.0
    assert res.observed["dispersion"] > res.replicated["dispersion"].max() and res.p_ge["dispersion"] == 0.0
    assert res.p_le["mean"] == 0.0 and res.n_marked == 0                                 # half the counts are gone from the mean too


def test_check_counts_and_reports_poisson_markers(gpu):
    d, rows, n = 2, 40, 6
    X = np.zeros((rows, d), np.float32)
    X[:, 0] = 1.0
    X[7, 0] = 100.0                                      # predictor 100 w_0: the rate overflows float32 where w_0 is near 1
    model = PoissonRegression(d)
    guide = AutoDiagonalNormal(model)
    params = {"auto_loc": np.array([1.0, 0.0], np.float32), "auto_scale": np.full(2, 1e-3, np.float32)}
    with pytest.warns(RuntimeWarning, match="Poisson marker"):
        res = ppc.posterior_predictive_check(key(4), n, model, (X, np.ones(rows, np.float32)), guide, params, statistics=("max",))
    assert res.n_marked == n and (res.replicated["max"] == INT_MAX).all() and res.p_ge["max"] == 1.0


# ------------------------------------------------------------------------------- the workspace contract
def _under_fill(fill, fn):
    rec = H.Recorder(fill, 0, None)
    mp = pytest.MonkeyPatch()
    H.guarded_empty(mp, ppc, rec, "rep_stats")
    try:
        st = fn()
        torch.cuda.synchronize()
    finally:
        mp.undo()
    rec.check_all(fill)
    assert len(rec.workspaces) == 1 and rec.workspaces[0].nbytes == R.strips(st.n_rows)[2] * 5 * max(st.sum.numel(), 1) * 8
    return [H.raw_bytes(x) for x in st._five()]


@pytest.mark.parametrize("which", ["rep_stats", "predict_stats_poisson", "predict_stats_linear", "predict_stats_logistic"])
def test_both_entries_ignore_what_the_workspace_held_and_stay_inside_it(gpu, which):
    rng = np.random.default_rng(12)
    d, rows, n = 3, 1000, 130                            # 8 strips, two draw tiles
    if which == "rep_stats":
        md = _dev(_random_matrix("float32", n, rows, 1))
        fn = lambda: ppc.replicate_stats(md, 0.5)
    else:
        model = _family_model(which.split("_")[-1], d, True)
        X = _dev(rng.uniform(-1, 1, size=(rows, d)).astype(np.float32))
        samples = {"w": _dev(rng.normal(size=(n, d)).astype(np.float32)), "intercept": _dev(rng.normal(size=n).astype(np.float32))}
        k = key(6)
        fn = lambda: ppc.predictive_stats(k, model, samples, X, shift=0.5)
    base = _under_fill("zero", fn)
    for fill in ("ones", "big", "bits"):
        got = _under_fill(fill, fn)
        assert all(torch.equal(a, b) for a, b in zip(base, got)), (which, fill)


# ------------------------------------------------------------------------------- refusals at the C boundary
def test_c_entries_refuse_before_any_launch_and_leave_the_outputs_alone(gpu):
    lib = L.load()
    d, rows, n = 3, 50, 4
    X, lat, ld, w_off, b_col, keys = _problem("linear", d, rows, n, False, 1)
    Xd, latd, kd = _dev(X), _dev(lat), _dev(keys)
    m = _dev(_random_matrix("float32", n, rows, 2))
    out = torch.full((5, n), -123.0, dtype=torch.float64, device=DEV)
    nbytes = lib.d3p_rep_stats_workspace(rows, n)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    s = L.stream_ptr()

    def rep(m_=m, dtype=0, ld_=rows, n_=n, rows_=rows, shift=0.0, out_=out, ws_=ws, nb=nbytes):
        return lib.d3p_rep_stats(s, L.ptr(m_), dtype, ld_, n_, rows_, shift, L.ptr(out_), L.ptr(ws_), nb)

    def fused(ms, rows_=rows, nb=nbytes, d_=d, shift=0.0):
        return lib.d3p_predict_stats(s, C.byref(ms), L.ptr(Xd), rows_, d_, L.ptr(latd), ld, w_off, b_col, n, L.ptr(kd), shift, L.ptr(out), L.ptr(ws), nb)

    assert rep(nb=nbytes - 1) == -1 and b"workspace" in lib.d3p_last_error()
    assert rep(rows_=0) == -1 and rep(ld_=rows - 1) == -1 and rep(dtype=2) == -1 and rep(dtype=-1) == -1 and rep(n_=0) == -1
    assert rep(shift=float("inf")) == -1 and rep(rows_=2 ** 32, ld_=2 ** 32) == -3
    assert rep(m_=torch.zeros(n, rows)) == -1 and b"device memory" in lib.d3p_last_error()          # a host pointer
    assert rep(out_=torch.zeros(5, n, dtype=torch.float64)) == -1 and rep(ws_=torch.zeros(nbytes, dtype=torch.uint8)) == -1
    ok = _model_struct("linear", d, False)
    assert fused(ok, nb=nbytes - 1) == -1 and b"workspace" in lib.d3p_last_error()
    assert fused(ok, rows_=0) == -1 and b"rows must be" in lib.d3p_last_error()
    assert fused(ok, d_=d + 1) == -1 and fused(ok, shift=float("nan")) == -1
    gauss = L.LogregModel(d, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_GAUSS_MEAN, L.D3P_GUIDE_SOFTPLUS, 1.0)
    assert fused(gauss) == -3 and b"Gaussian-mean" in lib.d3p_last_error()
    sites = L.LogregModel(d, 1, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LOGREG, L.D3P_GUIDE_EXP_SITES, 0.0)
    assert fused(sites) == -3 and b"D3P_GUIDE_EXP_SITES" in lib.d3p_last_error()
    bad_sigma = L.LogregModel(d, 0, 1.0, 1.0, 1.0, 1.0, L.D3P_FAMILY_LINREG, L.D3P_GUIDE_SOFTPLUS, 0.0)
    assert fused(bad_sigma) == -1
    torch.cuda.synchronize()
    assert bool((out == -123.0).all())                   # nothing was launched
    assert rep() == 0 and fused(ok) == 0                 # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert not bool((out == -123.0).any())


# ------------------------------------------------------------------------------- the example flag
def test_poisson_example_prints_the_check_of_its_zero_inflated_counts(gpu, capsys):
    """examples/poisson_regression.py --ppc 32 --zero-inflate 0.3 on a small table: the printed layout, the effect of --zero-inflate on
    the observed counts and the arithmetic of the printed tail shares.  30 % of 2000 counts are forced to 0 (600 +- 20, binomial), on
    top of the zeros the counts hold already: at least 500 observed.  Which verdict the check reaches is NOT asserted here: it
    depends on where 300 noisy DP-SVI steps leave the guide (which is not the maximum-likelihood fit), not on this module; the
    verdict's meaning is pinned by the two deterministic checks above."""
    import argparse
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "poisson_regression.py")
    spec = importlib.util.spec_from_file_location("poisson_regression_ppc_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(argparse.Namespace(sigma=0.5, clip_threshold=1.0, num_steps=300, learning_rate=2e-2, batch_size=200, dimensions=4,
                                num_samples=2000, ppc=32, zero_inflate=0.3))
    lines = capsys.readouterr().out.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("posterior predictive check (2000 rows, 32 replicated data sets")]
    assert len(at) == 1
    body = [l.split() for l in lines[at[0] + 1:at[0] + 7]]
    assert [b[:2] for b in body] == [["ppc", s] for s in ("mean", "sd", "min", "max", "zeros", "dispersion")]
    by_name = {b[1]: b for b in body}
    assert float(by_name["zeros"][3]) >= 500
    for b in body:
        p_ge, p_le = float(b[b.index("p_ge") + 1]), float(b[b.index("p_le") + 1])
        assert 0.0 <= p_ge <= 1.0 and 0.0 <= p_le <= 1.0 and p_ge + p_le >= 1.0 - 1e-3, b      # (ties count twice; three decimals printed)
        assert float(b[6].strip("[,")) <= float(b[7].strip("]")), b                            # the 90 % range, in order
