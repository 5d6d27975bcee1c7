"""Credible and predictive intervals on the GPU (d3p_col_quantiles, d3p_predict_mean_rows, d3p_amd.intervals) against
tests/quantiles_ref.py.  The selection is exact and the interpolation is float64 rounded once, so the quantile entry is compared BY
VALUE (NaN by class, -0 equal to +0), never within a tolerance.  Only d3p_predict_mean_rows and what is built on it carry a bound: that
of tests/moments_ref.py, whose link k_mean_rows restates (quantiles_ref.mean_rows / interval_bound)."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import loglik_ref as LR
from tests import moments_ref as MR
from tests import predictive_ref as P
from tests import quantiles_ref as QR

pytestmark = pytest.mark.gpu
CANARY = 12345.0
PAD = 64


def np_(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module")
def IV(gpu):
    from d3p_amd import intervals
    return intervals


@pytest.fixture(scope="module")
def S(gpu):
    import d3p_amd._lib as L
    return int(L.load().d3p_col_quantiles_staged_max())


def entry(m, pos, ld=None):
    """d3p_col_quantiles on the (n, cols) numpy matrix m at leading dimension ld and the positions [(lo, g)], canaries in the matrix's
    padding, between the output's rows (out_ld = cols + PAD) and around it: (Q, cols) numpy float32 after the canaries were checked."""
    import d3p_amd._lib as L
    n, cols = m.shape
    ld = cols if ld is None else ld
    Q = len(pos)
    is_int = m.dtype == np.int32
    mat = torch.full((n, ld), 12345 if is_int else CANARY, dtype=torch.int32 if is_int else torch.float32, device="cuda")
    mat[:, :cols] = torch.tensor(m).cuda()
    out_ld = cols + PAD
    out = torch.full((PAD + Q * out_ld,), CANARY, device="cuda")
    lo = (C.c_uint32 * Q)(*[p[0] for p in pos])
    g = (C.c_double * Q)(*[p[1] for p in pos])
    L.check(L.load().d3p_col_quantiles(L.stream_ptr(), L.ptr(mat), int(is_int), ld, n, cols, Q, lo, g, L.ptr(out[PAD:]), out_ld))
    torch.cuda.synchronize()
    body = out[PAD:].reshape(Q, out_ld)
    assert bool((out[:PAD] == CANARY).all()) and bool((body[:, cols:] == CANARY).all()), "the output was written outside its extent"
    assert np.array_equal(bits(np_(mat[:, :cols])), bits(m)) and bool((mat[:, cols:] == (12345 if is_int else CANARY)).all())
    return np_(body[:, :cols]).copy()


def assert_same(got, want, what):
    assert QR.same_values(got, want), f"{what}: (q, column) {QR.first_difference(got, want)}"


# ---------------------------------------------------------------- 1. the entry alone against the reference
@pytest.mark.parametrize("n_spec", [1, 2, 3, 31, 128, 257, "S", "S+1", 1500])
def test_direct_entry_equals_the_reference_by_value(gpu, S, n_spec):
    """Every kind of matrix at cols around the workgroup's 32 columns, ld = cols + 64 and ld = cols, all eight probabilities; n around
    the draw lanes' 8, and S | S + 1: the last staged and the first streamed draw count."""
    n = {"S": S, "S+1": S + 1}.get(n_spec, n_spec)
    pos = QR.positions(QR.PROBS, n)
    for cols in (1, 31, 32, 33, 300):
        for kind in QR.KINDS:
            m = QR.matrix(kind, n, cols)
            want = QR.quantiles_at(m, pos)
            for ld in (cols + 64, cols):
                assert_same(entry(m, pos, ld), want, f"{kind} n={n} cols={cols} ld={ld}")


def test_direct_entry_at_the_largest_n(gpu):
    n, cols = 65535, 33
    pos = QR.positions(QR.PROBS, n)
    for kind in ("normal", "counts"):
        m = QR.matrix(kind, n, cols)
        assert_same(entry(m, pos, cols + 64), QR.quantiles_at(m, pos), f"{kind} n=65535")


# ---------------------------------------------------------------- 2. path independence
def test_a_columns_bits_do_not_depend_on_path_neighbours_or_ld(gpu, S):
    """Staged against streamed: the S draws of every column get one more draw above all of them, which makes the launch stream (n = S
    + 1) and leaves the (lo+1)-th and (lo+2)-th smallest values of every requested position where they were, so the SAME (lo, g) must
    give the same bits.  Alone against among 299 other columns, and two leading dimensions, on both paths."""
    cols = 300
    pos = QR.positions(QR.PROBS, S)
    for kind in ("normal", "quarters", "counts"):
        m = QR.matrix(kind, S, cols)
        top = np.full((1, cols), QR.INT32_MAX if m.dtype == np.int32 else 3.0e38, m.dtype)
        if m.dtype == np.int32:
            m = np.minimum(m, QR.INT32_MAX - 1)                       # (the added draw lies strictly above)
        staged = entry(m, pos, cols + 64)
        more = np.concatenate([m[:5], top, m[5:]], axis=0)
        assert more.shape[0] == S + 1
        streamed = entry(more, pos, cols + 64)
        assert np.array_equal(bits(staged), bits(streamed)), f"{kind}: the staged and the streamed path differ"
        assert_same(staged, QR.quantiles_at(m, pos), kind)
        for mat, whole in ((m, staged), (more, streamed)):
            assert np.array_equal(bits(entry(mat, pos, cols)), bits(whole)), f"{kind}: ld changes the bits"
            for c in (0, 123, 299):
                alone = entry(np.ascontiguousarray(mat[:, c:c + 1]), pos, 1)
                assert np.array_equal(bits(alone[:, 0]), bits(whole[:, c])), f"{kind}: column {c} alone differs"
            again = entry(mat, pos, cols + 64)
            assert np.array_equal(bits(again), bits(whole)), "two calls differ"


# ---------------------------------------------------------------- 3. fixed columns
def test_non_finite_table_on_the_device(gpu):
    for col, lo, g, want in QR.NONFINITE:
        got = entry(np.array(col, np.float32).reshape(-1, 1), [(lo, g)])
        assert_same(got, np.array([[want]], np.float32), f"{col} at ({lo}, {g})")


@pytest.mark.parametrize("n_spec", [31, "S+1"])
def test_a_nan_makes_its_column_nan_and_no_other(gpu, S, n_spec):
    n = S + 1 if n_spec == "S+1" else n_spec
    pos = QR.positions(QR.PROBS, n)
    m = QR.matrix("normal", n, 70)
    clean = entry(m, pos)
    m2 = m.copy()
    m2[n // 2, 33] = np.nan
    m2[0, 69] = -np.nan
    m2[3, 5], m2[4, 5], m2[9, 6] = -np.inf, np.inf, np.inf
    got = entry(m2, pos, 70 + 64)
    assert np.isnan(got[:, 33]).all() and np.isnan(got[:, 69]).all()
    keep = [c for c in range(70) if c not in (5, 6, 33, 69)]
    assert np.array_equal(bits(got[:, keep]), bits(clean[:, keep]))
    assert_same(got, QR.quantiles_at(m2, pos), "infinite draws")
    assert got[0, 5] == -np.inf and got[-1, 5] == np.inf and got[-1, 6] == np.inf and np.isfinite(got[0, 6])


def test_negative_and_positive_zero_are_one_value(gpu):
    m = np.array([[-0.0, 0.0, 1.0], [0.0, -0.0, -0.0], [-0.0, -0.0, 0.0], [0.0, 0.0, -1.0]], np.float32)
    got = entry(m, QR.positions(QR.PROBS, 4))
    assert np.all(got[:, :2] == 0.0) and not np.signbit(got[:, :2]).any()     # +0 is what the key stands for
    assert_same(got, QR.quantiles(m, QR.PROBS), "zeros")


# ---------------------------------------------------------------- 4. refusals
def test_col_quantiles_refuses_as_declared(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    n, cols = 9, 40
    mat = torch.zeros((n, cols), device="cuda")
    out = torch.full((2, cols), CANARY, device="cuda")
    lo2, g2 = (C.c_uint32 * 2)(0, 4), (C.c_double * 2)(0.0, 0.5)

    def run(mat_=L.ptr(mat), dtype=0, ld=cols, n_=n, cols_=cols, Q=2, lo=lo2, g=g2, out_=L.ptr(out), out_ld=cols):
        return lib.d3p_col_quantiles(L.stream_ptr(), mat_, dtype, ld, n_, cols_, Q, lo, g, out_, out_ld)
    odd = C.c_void_p(out.data_ptr() + 2)
    assert run(mat_=None) == -1 and run(out_=None) == -1 and run(lo=None) == -1 and run(g=None) == -1
    assert run(out_=odd) == -1 and b"aligned" in lib.d3p_last_error()
    assert run(mat_=C.c_void_p(mat.data_ptr() + 1)) == -1
    assert run(n_=0) == -1 and run(n_=65536) == -1 and b"65535" in lib.d3p_last_error()
    assert run(Q=0) == -1 and run(Q=9) == -1 and b"Q" in lib.d3p_last_error()
    assert run(lo=(C.c_uint32 * 2)(0, 9)) == -1 and b"lo" in lib.d3p_last_error()
    assert run(g=(C.c_double * 2)(0.0, 1.0)) == -1 and run(g=(C.c_double * 2)(-0.1, 0.0)) == -1
    assert run(g=(C.c_double * 2)(float("nan"), 0.0)) == -1
    assert run(lo=(C.c_uint32 * 2)(0, 8), g=(C.c_double * 2)(0.0, 0.25)) == -1 and b"n - 1" in lib.d3p_last_error()
    assert run(ld=cols - 1) == -1 and run(out_ld=cols - 1) == -1 and b"out_ld" in lib.d3p_last_error()
    assert run(dtype=2) == -1 and run(dtype=-1) == -1 and b"dtype" in lib.d3p_last_error()
    host = torch.zeros((n, cols))
    assert run(mat_=L.ptr(host)) == -1 and b"device memory" in lib.d3p_last_error()
    assert run(out_=L.ptr(torch.zeros((2, cols)))) == -1
    assert run(cols_=32 * (2 ** 31 - 1) + 1, ld=2 ** 40, out_ld=2 ** 40) == -3          # D3P_E_UNSUPPORTED
    assert run(cols_=0) == 0
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())                                 # nothing was launched
    assert run() == 0
    assert run(lo=(C.c_uint32 * 2)(8, 8), g=(C.c_double * 2)(0.0, 0.0)) == 0            # lo = n - 1 with g = 0 is p = 1
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


def _struct(model, d):
    from d3p_amd import infer_util as U
    return U._model_struct(model, U._family(model), d)


def test_predict_mean_rows_refuses_as_declared(gpu):
    import d3p_amd._lib as L
    lib = L.load()
    n, rows, d = 5, 40, 4
    X, lat = torch.zeros((rows, d), device="cuda"), torch.zeros((n, d + 1), device="cuda")
    out = torch.full((n, rows), CANARY, device="cuda")
    ms = _struct(make_model("poisson", d, True), d)

    def run(ms_=ms, X_=L.ptr(X), rows_=rows, lat_=L.ptr(lat), ld=d + 1, w_off=0, b_col=d, n_=n, out_=L.ptr(out), out_ld=rows):
        return lib.d3p_predict_mean_rows(L.stream_ptr(), C.byref(ms_), X_, rows_, lat_, ld, w_off, b_col, n_, out_, out_ld)
    gauss = _struct(make_model("poisson", d, False), d)
    gauss.family, gauss.lik_sigma = L.D3P_FAMILY_GAUSS_MEAN, 1.0
    sites = _struct(make_model("logistic", d, True), d)
    sites.guide_transform = L.D3P_GUIDE_EXP_SITES
    assert run(ms_=gauss, b_col=-1) == -3 and run(ms_=sites) == -3                        # D3P_E_UNSUPPORTED
    assert run(X_=None) == -1 and run(lat_=None) == -1 and run(out_=None) == -1
    assert run(n_=0) == -1 and run(ld=d) == -1 and run(b_col=-1) == -1 and run(b_col=1) == -1 and run(w_off=2) == -1
    assert run(out_ld=rows - 1) == -1 and b"out_ld" in lib.d3p_last_error()
    assert run(X_=L.ptr(torch.zeros((rows, d)))) == -1 and b"device memory" in lib.d3p_last_error()
    bad_sigma = _struct(make_model("linear", d, True), d)
    bad_sigma.lik_sigma = 0.0
    assert run(ms_=bad_sigma) == -1
    assert run(rows_=0, out_ld=0) == 0
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())                                 # nothing was launched
    assert run() == 0
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())                                    # exp(0)


# ---------------------------------------------------------------- 5. d3p_predict_mean_rows against moments_ref
def make_model(family, d, intercept):
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    if family == "logistic":
        return LogisticRegression(d, intercept=intercept)
    if family == "linear":
        return LinearRegression(d, intercept=intercept, obs_scale=MR.SIGMA["linear"])
    return PoissonRegression(d, intercept=intercept)


def samples_of(W, b):
    s = {"w": torch.tensor(np.array(W)).cuda()}
    if b is not None:
        s["intercept"] = torch.tensor(np.array(b)).cuda()
    return s


def mean_rows(family, X, W, b, pad=3):
    """d3p_predict_mean_rows at out_ld = rows + pad with canaries in the padding: (n, rows) numpy float32."""
    import d3p_amd._lib as L
    n, d = W.shape
    rows = X.shape[0]
    lat = torch.tensor(W if b is None else np.concatenate([W, np.asarray(b).reshape(n, 1)], axis=1)).cuda().contiguous()
    Xt = torch.tensor(X).cuda()
    out = torch.full((n, rows + pad), CANARY, device="cuda")
    ms = _struct(make_model(family, d, b is not None), d)
    L.check(L.load().d3p_predict_mean_rows(L.stream_ptr(), C.byref(ms), L.ptr(Xt), rows, L.ptr(lat), lat.shape[1], 0, d if b is not None else -1, n,
                                           L.ptr(out), rows + pad))
    torch.cuda.synchronize()
    assert bool((out[:, rows:] == CANARY).all()), "the matrix was written outside its extent"
    return np_(out[:, :rows]).copy()


@pytest.mark.parametrize("family,n,rows,d,intercept", MR.sweep_cases())
def test_mean_rows_at_tile_edges(gpu, family, n, rows, d, intercept):
    from d3p_amd import prediction as Pm
    X, _, W, b = LR.inputs(family, n, rows, d, intercept)
    got = mean_rows(family, X, W, b)
    mu, e = QR.mean_rows(family, X, W, b, MR.SIGMA[family])
    assert np.isfinite(mu).all()
    MR.assert_close(got, mu, e, f"{family} n={n} rows={rows} d={d} intercept={intercept} mu")
    pm = np_(Pm.predictive_moments(make_model(family, d, intercept), samples_of(W, b), torch.tensor(X).cuda())["mean"])
    b_mean, _ = MR.bounds(family, X, W, b, MR.SIGMA[family])
    MR.assert_close(got.astype(np.float64).mean(axis=0), pm.astype(np.float64), b_mean, "the mean over the draws against predictive_moments")


@pytest.mark.parametrize("all_draws", [False, True])
def test_mean_rows_poisson_overflow_by_class(gpu, all_draws):
    X, W, t = MR.overflow_problem(all_draws)
    got = mean_rows("poisson", X, W, None)
    mu, e = QR.mean_rows("poisson", X, W, None, 1.0)
    assert np.isposinf(mu).any() and not np.isnan(got).any()
    MR.assert_close(got, mu, np.where(np.isfinite(mu), e, 0.0), f"overflow all_draws={all_draws}")


def test_mean_rows_keeps_a_nan_predictor(gpu):
    X, _, W, b = LR.inputs("logistic", 3, 5, 4, True)
    W = W.copy()
    W[1, 2] = np.nan
    for family in MR.FAMILIES:
        got = mean_rows(family, X, W, b)
        assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()


# ---------------------------------------------------------------- 6. credible_interval end to end
@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("d", [4, 33])
@pytest.mark.parametrize("family", MR.FAMILIES)
def test_credible_interval(IV, family, d, intercept):
    n, rows = 64, 129
    X, y, W, b = LR.inputs(family, n, rows, d, intercept)
    model, Xt, s = make_model(family, d, intercept), torch.tensor(X).cuda(), samples_of(W, b)
    res = IV.credible_interval(model, s, Xt, torch.tensor(y).cuda(), rows, probs=QR.PROBS)
    assert sorted(res) == ["quantiles"]
    q = res["quantiles"]
    assert q.shape == (len(QR.PROBS), rows) and q.dtype == torch.float32 and q.is_cuda
    mu, e = QR.mean_rows(family, X, W, b, MR.SIGMA[family])
    ref64 = np.quantile(mu, QR.PROBS, axis=0, method="linear")      # (the rule on the float64 mu, unrounded: the rounding is in the bound)
    bound = QR.interval_bound(ref64, e)
    err = np.abs(np_(q).astype(np.float64) - ref64)
    print(f"{family} d={d} intercept={intercept}: largest error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    written = torch.tensor(mean_rows(family, X, W, b)).cuda()
    assert_same(np_(q), np_(IV.quantiles(written, QR.PROBS)), "credible_interval against quantiles of d3p_predict_mean_rows' matrix")
    assert_same(np_(q), QR.quantiles(np_(written), QR.PROBS), "and against the reference rule on that matrix")
    named = IV.credible_interval(model, s, Xt, prob=0.9)
    assert sorted(named) == ["lower", "median", "upper"] and all(v.shape == (rows,) for v in named.values())
    three = np_(IV.credible_interval(model, s, Xt, probs=((1.0 - 0.9) / 2.0, 0.5, (1.0 + 0.9) / 2.0))["quantiles"])   # (prob = 0.9 in floats)
    assert all(np.array_equal(bits(np_(named[k])), bits(three[i])) for i, k in enumerate(("lower", "median", "upper")))
    assert bool((named["lower"] <= named["median"]).all()) and bool((named["median"] <= named["upper"]).all())


def test_posterior_credible_interval_draws_the_latents_of_the_predictive(IV):
    from d3p_amd import predictive as PS
    from d3p_amd.models import AutoDiagonalNormal
    n, rows, d = 30, 70, 4
    for family in MR.FAMILIES:
        X, _, _, _ = LR.inputs(family, 1, rows, d, True, seed=41)
        model = make_model(family, d, True)
        guide = AutoDiagonalNormal(model)
        params = {k: torch.tensor(v) for k, v in P.logreg_params(guide, d, True, np.random.default_rng(12)).items()}
        params["auto_loc"] = 0.2 * params["auto_loc"]             # (keeps the Poisson rates moderate)
        Xt, key = torch.tensor(X).cuda(), P.key(77)
        draws = PS.posterior_predictive_samples(key, n, model, (Xt,), guide, params)
        want = IV.credible_interval(model, {"w": draws["w"], "intercept": draws["intercept"]}, Xt)
        got = IV.posterior_credible_interval(key, n, model, (Xt,), guide, params)
        assert all(np.array_equal(bits(np_(got[k])), bits(np_(want[k]))) for k in ("lower", "median", "upper"))
        other = IV.posterior_credible_interval(P.key(78), n, model, (Xt,), guide, params)
        assert not torch.equal(other["median"], got["median"])


# ---------------------------------------------------------------- 7. predictive intervals
@pytest.mark.parametrize("family", ["linear", "poisson"])
def test_predictive_intervals_equal_the_rule_on_the_sampled_outcomes(IV, family):
    from d3p_amd import predictive as PS
    from d3p_amd.models import AutoDiagonalNormal
    n, rows, d = 100, 300, 4
    X, _, W, b = LR.inputs(family, n, rows, d, True, seed=61)
    model, Xt, s, key = make_model(family, d, True), torch.tensor(X).cuda(), samples_of(W, b), P.key(5)
    obs = PS.predictive_samples(key, model, s, Xt)
    assert obs.dtype == (torch.float32 if family == "linear" else torch.int32) and obs.shape == (n, rows)
    got = IV.predictive_interval(key, model, s, Xt, probs=QR.PROBS)["quantiles"]
    assert_same(np_(got), QR.quantiles(np_(obs), QR.PROBS), f"{family} predictive_interval")
    named = IV.predictive_interval(key, model, s, Xt, prob=0.8)
    assert_same(np.stack([np_(named[k]) for k in ("lower", "median", "upper")]), QR.quantiles(np_(obs), ((1.0 - 0.8) / 2.0, 0.5, (1.0 + 0.8) / 2.0)), "named")
    guide = AutoDiagonalNormal(model)
    params = {k: torch.tensor(v) for k, v in P.logreg_params(guide, d, True, np.random.default_rng(12)).items()}
    params["auto_loc"] = 0.2 * params["auto_loc"]                 # (keeps the Poisson rates moderate)
    pobs = PS.posterior_predictive_samples(key, n, model, (Xt,), guide, params)["obs"]
    pgot = IV.posterior_predictive_interval(key, n, model, (Xt,), guide, params, probs=QR.PROBS)["quantiles"]
    assert_same(np_(pgot), QR.quantiles(np_(pobs), QR.PROBS), f"{family} posterior_predictive_interval")
    with pytest.raises(TypeError, match="credible_interval"):
        IV.predictive_interval(key, make_model("logistic", d, True), s, Xt)


# ---------------------------------------------------------------- 8. slabs
def test_slabs_give_the_bits_of_one_call(IV):
    """rows = 300 at 128 rows per slab: 128, 128 and 44 rows.  The predictive forms write their matrix whole (d3p_predict_glm has no
    row offset): the default fits, the two small values are refused with the bytes that are needed."""
    n, rows, d = 100, 300, 33
    for family in MR.FAMILIES:
        X, _, W, b = LR.inputs(family, n, rows, d, True, seed=51)
        model, Xt, s = make_model(family, d, True), torch.tensor(X).cuda(), samples_of(W, b)
        whole = np_(IV.credible_interval(model, s, Xt, probs=QR.PROBS)["quantiles"])
        assert np.isfinite(whole).all()
        for slab_bytes in (4 * n * 128, 1, 4 * n * 128 + 100):
            part = np_(IV.credible_interval(model, s, Xt, probs=QR.PROBS, slab_bytes=slab_bytes)["quantiles"])
            assert np.array_equal(bits(part), bits(whole)), f"{family}: slab_bytes={slab_bytes} changes the bits"
        if family != "logistic":
            key = P.key(9)
            one = np_(IV.predictive_interval(key, model, s, Xt, probs=QR.PROBS)["quantiles"])
            fit = np_(IV.predictive_interval(key, model, s, Xt, probs=QR.PROBS, slab_bytes=4 * n * rows)["quantiles"])
            assert np.array_equal(bits(one), bits(fit))
            for slab_bytes in (4 * n * 128, 1):
                with pytest.raises(ValueError, match=rf"slab_bytes >= {4 * n * rows}\b"):
                    IV.predictive_interval(key, model, s, Xt, probs=QR.PROBS, slab_bytes=slab_bytes)


# ---------------------------------------------------------------- 9. latent_summary
def test_latent_summary(IV):
    import d3p_amd._lib as L
    n, d = 257, 33
    rng = np.random.default_rng(8)
    lat = torch.tensor((rng.normal(size=(n, d + 1)) * 10.0 ** rng.integers(-2, 3, size=d + 1)).astype(np.float32)).cuda()
    s = {"w": lat[:, :d], "intercept": lat[:, d]}                    # packed views, as the predictive forms return them
    res = IV.latent_summary(s, prob=0.9)
    assert sorted(res) == ["intercept", "w"] and all(sorted(v) == ["lower", "mean", "median", "std", "upper"] for v in res.values())
    assert res["w"]["mean"].shape == (d,) and res["intercept"]["mean"].shape == () and res["w"]["median"].dtype == torch.float32
    stats = torch.empty((4, d + 1), dtype=torch.float64, device="cuda")
    L.check(L.load().d3p_col_stats(L.stream_ptr(), L.ptr(lat), d + 1, n, d + 1, L.ptr(stats)))
    for name, cols in (("w", slice(0, d)), ("intercept", d)):
        r, host = res[name], np_(lat)[:, cols].reshape(n, -1)
        assert np.array_equal(np_(r["mean"]).reshape(-1).view(np.int64), np_(stats[0, cols]).reshape(-1).view(np.int64))
        assert np.array_equal(np_(r["std"]).reshape(-1).view(np.int64), np_(torch.sqrt(stats[1, cols])).reshape(-1).view(np.int64))
        want = np.quantile(host.astype(np.float64), ((1.0 - 0.9) / 2.0, 0.5, (1.0 + 0.9) / 2.0), axis=0, method="linear").astype(np.float32)
        assert_same(np.stack([np_(r[k]).reshape(-1) for k in ("lower", "median", "upper")]), want, name)
        assert np.allclose(np_(r["mean"]).reshape(-1), host.astype(np.float64).mean(axis=0), rtol=1e-12, atol=0)
        assert np.allclose(np_(r["std"]).reshape(-1), host.astype(np.float64).std(axis=0, ddof=1), rtol=1e-10, atol=0)
    one = IV.latent_summary({"w": np_(lat)[:1, :d]})["w"]               # n = 1 from a numpy array: std is NaN, the quantiles the draw
    assert bool(torch.isnan(one["std"]).all()) and np.array_equal(np_(one["median"]), np_(lat)[0, :d])


# ---------------------------------------------------------------- 10. examples
def _example(name):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ex_intervals_" + name, os.path.join(root, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["linear_regression", "poisson_regression"])
def test_examples_report_intervals_behind_their_flag(IV, capsys, name):
    mod = _example(name)
    base = dict(sigma=0.5, clip_threshold=1.0, num_steps=300, learning_rate=2e-2, batch_size=200, dimensions=4, num_samples=2000, obs_scale=0.5)
    mod.main(argparse.Namespace(intervals=50, **base))
    out = capsys.readouterr().out
    m = re.search(r"90% predictive interval \(2000 rows, 50 draws\): coverage ([\d.]+), mean width ([\d.]+)", out)
    assert m, out
    coverage, width = float(m.group(1)), float(m.group(2))
    assert 0.0 <= coverage <= 1.0 and np.isfinite(width) and width > 0.0
    rows = re.findall(r"w\[(\d)\]: mean (-?[\d.]+), std ([\d.]+), median (-?[\d.]+), 5% (-?[\d.]+), 95% (-?[\d.]+)", out)
    assert [r[0] for r in rows] == ["0", "1", "2", "3"]
    assert all(float(r[4]) <= float(r[3]) <= float(r[5]) and float(r[2]) > 0.0 for r in rows)
    mod.main(argparse.Namespace(**base))
    plain = capsys.readouterr().out
    assert "predictive interval" not in plain and "w[0]" not in plain and "loss per example" in plain
