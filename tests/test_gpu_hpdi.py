"""Highest-density intervals on the GPU (d3p_col_hpdi, d3p_amd.intervals.hpdi, kind="hpdi", interval="hpdi") against tests/hpdi_ref.py.
The sort is exact, a float32 length is one float32 subtraction, an int32 length an integer, and the ends are stored values: everything
is compared BY VALUE (NaN by class, -0 equal to +0) or bit for bit, never within a tolerance."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import hpdi_ref as HR
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
def FORMS(gpu):
    """(N32, N8, Nmax): the largest n of the 32-column form, of the 8-column form, and d3p_col_hpdi_max_n(), from the query functions."""
    import d3p_amd._lib as L
    lib = L.load()
    nmax = int(lib.d3p_col_hpdi_max_n())

    def largest(form):
        lo, hi = 1, nmax                                  # cols_per_group falls with n: the largest n that still gives `form` or wider
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if lib.d3p_col_hpdi_cols_per_group(mid) >= form else (lo, mid - 1)
        assert lib.d3p_col_hpdi_cols_per_group(lo) == form and lib.d3p_col_hpdi_cols_per_group(lo + 1) < form
        return lo
    n32, n8 = largest(32), largest(8)
    assert n32 < n8 < nmax and lib.d3p_col_hpdi_cols_per_group(nmax) == 2 and lib.d3p_col_hpdi_cols_per_group(nmax + 1) == 0
    return n32, n8, nmax


def entry(m, lens, ld=None):
    """d3p_col_hpdi on the (n, cols) numpy matrix m at leading dimension ld and the window lengths, canaries in the matrix's padding,
    between the output's rows (out_ld = cols + PAD) and around it: (2 Q, cols) numpy float32 after the canaries were checked."""
    import d3p_amd._lib as L
    n, cols = m.shape
    ld = cols if ld is None else ld
    Q = len(lens)
    is_int = m.dtype == np.int32
    mat = torch.full((n, ld), 12345 if is_int else CANARY, dtype=torch.int32 if is_int else torch.float32, device="cuda")
    mat[:, :cols] = torch.tensor(m).cuda()
    out_ld = cols + PAD
    out = torch.full((PAD + 2 * Q * out_ld + PAD,), CANARY, device="cuda")
    L.check(L.load().d3p_col_hpdi(L.stream_ptr(), L.ptr(mat), int(is_int), ld, n, cols, Q, (C.c_uint32 * Q)(*lens), L.ptr(out[PAD:]), out_ld))
    torch.cuda.synchronize()
    body = out[PAD:PAD + 2 * Q * out_ld].reshape(2 * Q, out_ld)
    assert bool((out[:PAD] == CANARY).all()) and bool((out[PAD + 2 * Q * out_ld:] == CANARY).all()) and bool((body[:, cols:] == CANARY).all()), \
        "the output was written outside its extent"
    assert np.array_equal(bits(np_(mat[:, :cols])), bits(m)) and bool((mat[:, cols:] == (12345 if is_int else CANARY)).all())
    return np_(body[:, :cols]).copy()


def assert_same(got, want, what):
    assert QR.same_values(got, want), f"{what}: (row, column) {QR.first_difference(got, want)}"


# ---------------------------------------------------------------- 1. the entry alone against the comparator
@pytest.mark.parametrize("n_spec", [1, 2, 3, 9, 31, 128, 257, 1024, 1025, "N32", "N32+1", "N8", "N8+1"])
def test_direct_entry_equals_the_comparator_by_value(gpu, FORMS, n_spec):
    """Every kind of matrix at cols around the three forms' 32, 8 and 2 columns, ld = cols and ld = cols + 64, all window lengths of the
    sweep in one launch; n around the network's powers of two and on both sides of each form's limit."""
    n32, n8, _ = FORMS
    n = {"N32": n32, "N32+1": n32 + 1, "N8": n8, "N8+1": n8 + 1}.get(n_spec, n_spec)
    lens = HR.sweep_lengths(n)
    for cols in (1, 7, 8, 9, 31, 32, 33, 300):
        for kind in HR.KINDS:
            m = HR.matrix(kind, n, cols)
            want = HR.hpdi_at(m, lens)
            for ld in (cols, cols + 64):
                assert_same(entry(m, lens, ld), want, f"{kind} n={n} cols={cols} ld={ld} lengths {lens}")


def test_direct_entry_at_the_largest_n(gpu, FORMS):
    nmax = FORMS[2]
    lens = HR.sweep_lengths(nmax)
    for kind in ("normal", "counts"):
        for cols in (1, 2, 3, 33):
            m = HR.matrix(kind, nmax, cols)
            assert_same(entry(m, lens, cols + 64), HR.hpdi_at(m, lens), f"{kind} n={nmax} cols={cols}")


def test_two_tied_windows_the_first_wins(gpu):
    for n in (31, 257, 1025):
        L0, a1, _ = HR.two_windows_plan(n)
        m = HR.matrix("two_windows", n, 33)
        s = np.sort(m, axis=0)
        got = entry(m, [L0])
        assert np.array_equal(got[0], s[a1]) and np.array_equal(got[1], s[a1 + L0])


# ---------------------------------------------------------------- 2. form independence, neighbours, ld, repeats
@pytest.mark.parametrize("which", ["N32", "N8"])
def test_a_columns_bits_do_not_depend_on_form_neighbours_or_ld(gpu, FORMS, which):
    """One more draw above all the others moves a launch to the next narrower form and leaves s[0 .. n - 1] where they were.  At the SAME
    window lengths every window of the smaller matrix is a window of the larger one, which has exactly one more: the last one, which ends
    at the added draw -- 3e38, or INT32_MAX with the other counts capped one below -- and is on these matrices no shorter than the
    windows before it, so the first minimum stays where it was and the two forms must give the same bits (the comparator is held against
    both).  Alone against among 299 other columns, two leading dimensions and two calls, in both forms."""
    import d3p_amd._lib as L
    n = FORMS[0] if which == "N32" else FORMS[1]
    lib = L.load()
    assert lib.d3p_col_hpdi_cols_per_group(n) > lib.d3p_col_hpdi_cols_per_group(n + 1) > 0
    cols = 300
    lens = HR.sweep_lengths(n)
    for kind in ("normal", "quarters", "counts", "lognormal"):
        m = HR.matrix(kind, n, cols)
        top = np.full((1, cols), QR.INT32_MAX if m.dtype == np.int32 else 3.0e38, m.dtype)
        if m.dtype == np.int32:
            m = np.minimum(m, QR.INT32_MAX - 1)                       # (the added draw lies strictly above)
        wide = entry(m, lens, cols + 64)
        more = np.concatenate([m[:5], top, m[5:]], axis=0)
        assert more.shape[0] == n + 1
        narrow = entry(more, lens, cols + 64)
        assert_same(wide, HR.hpdi_at(m, lens), f"{kind} n={n}")
        assert_same(narrow, HR.hpdi_at(more, lens), f"{kind} n={n + 1}")
        assert np.array_equal(bits(wide), bits(narrow)), f"{kind}: the two forms differ"
        for mat, whole in ((m, wide), (more, narrow)):
            assert np.array_equal(bits(entry(mat, lens, cols)), bits(whole)), f"{kind}: ld changes the bits"
            for c in (0, 123, 299):
                alone = entry(np.ascontiguousarray(mat[:, c:c + 1]), lens, 1)
                assert np.array_equal(bits(alone[:, 0]), bits(whole[:, c])), f"{kind}: column {c} alone differs"
            again = entry(mat, lens, cols + 64)
            assert np.array_equal(bits(again), bits(whole)), "two calls differ"


# ---------------------------------------------------------------- 3. fixed columns, NaN, zeros
def test_fixed_columns_on_the_device(gpu):
    for col, L_, want in HR.FIXED:
        m = np.array(col, np.int32 if isinstance(col[0], int) else np.float32).reshape(-1, 1)
        assert_same(entry(m, [L_])[:, 0], np.array(want, np.float32), f"{col} at L={L_}")
    m = np.array(HR.INF_COLUMN, np.float32).reshape(-1, 1)
    got = entry(m, [L_ for L_, _ in HR.INF_TABLE])
    assert_same(got[:, 0], np.array([v for _, w in HR.INF_TABLE for v in w], np.float32), "the infinite column, every L in one launch")


@pytest.mark.parametrize("n_spec", [31, "N32+1", "N8+1"])
def test_a_nan_makes_its_column_nan_and_no_other(gpu, FORMS, n_spec):
    n = {"N32+1": FORMS[0] + 1, "N8+1": FORMS[1] + 1}.get(n_spec, n_spec)
    lens = HR.sweep_lengths(n)
    m = HR.matrix("normal", n, 70)
    clean = entry(m, lens)
    m2 = m.copy()
    m2[n // 2, 33] = np.nan
    m2[0, 69] = -np.nan
    m2[3, 5], m2[4, 5], m2[9, 6] = -np.inf, np.inf, np.inf
    got = entry(m2, lens, 70 + 64)
    assert np.isnan(got[:, 33]).all() and np.isnan(got[:, 69]).all()
    keep = [c for c in range(70) if c not in (5, 6, 33, 69)]
    assert not np.isnan(got[:, keep]).any() and np.array_equal(bits(got[:, keep]), bits(clean[:, keep]))
    assert_same(got, HR.hpdi_at(m2, lens), "infinite draws")


def test_negative_and_positive_zero_are_one_value(gpu):
    m = np.array([[-0.0, 0.0, 1.0], [0.0, -0.0, -0.0], [-0.0, -0.0, 0.0], [0.0, 0.0, -1.0]], np.float32)
    lens = HR.sweep_lengths(4)
    got = entry(m, lens)
    assert np.all(got[:, :2] == 0.0) and not np.signbit(got[:, :2]).any()     # +0 is what the key stands for
    assert_same(got, HR.hpdi_at(m, lens), "zeros")
    flipped = entry(-m, lens)
    assert np.array_equal(bits(flipped[:, :2]), bits(got[:, :2]))


# ---------------------------------------------------------------- 4. refusals
def test_col_hpdi_refuses_as_declared(gpu, FORMS):
    import d3p_amd._lib as L
    lib = L.load()
    nmax = FORMS[2]
    n, cols = 9, 40
    mat = torch.zeros((n, cols), device="cuda")
    out = torch.full((4, cols), CANARY, device="cuda")
    len2 = (C.c_uint32 * 2)(0, 4)

    def run(mat_=L.ptr(mat), dtype=0, ld=cols, n_=n, cols_=cols, Q=2, lens=len2, out_=L.ptr(out), out_ld=cols):
        return lib.d3p_col_hpdi(L.stream_ptr(), mat_, dtype, ld, n_, cols_, Q, lens, out_, out_ld)
    assert run(mat_=None) == -1 and run(out_=None) == -1 and run(lens=None) == -1 and b"null" in lib.d3p_last_error()
    assert run(out_=C.c_void_p(out.data_ptr() + 2)) == -1 and b"aligned" in lib.d3p_last_error()
    assert run(mat_=C.c_void_p(mat.data_ptr() + 1)) == -1
    assert run(dtype=2) == -1 and run(dtype=-1) == -1 and b"dtype" in lib.d3p_last_error()
    assert run(n_=0) == -1 and b"n >= 1" in lib.d3p_last_error()
    assert run(Q=0) == -1 and run(Q=9) == -1 and b"Q" in lib.d3p_last_error()
    assert run(lens=(C.c_uint32 * 2)(0, 9)) == -1 and b"len[1]" in lib.d3p_last_error()
    assert run(lens=(C.c_uint32 * 2)(2 ** 32 - 1, 0)) == -1
    dev_lens = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert run(lens=C.cast(C.c_void_p(dev_lens.data_ptr()), C.POINTER(C.c_uint32))) == -1 and b"host memory" in lib.d3p_last_error()
    assert run(ld=cols - 1) == -1 and run(out_ld=cols - 1) == -1 and b"out_ld" in lib.d3p_last_error()
    host = torch.zeros((n, cols))
    assert run(mat_=L.ptr(host)) == -1 and b"device memory" in lib.d3p_last_error()
    assert run(out_=L.ptr(torch.zeros((4, cols)))) == -1
    assert run(n_=nmax + 1) == -3 and str(nmax).encode() in lib.d3p_last_error()       # D3P_E_UNSUPPORTED: there is no streamed form
    assert run(n_=nmax + 1, cols_=0) == -3 and run(n_=2 ** 32 - 1) == -3
    assert run(cols_=32 * (2 ** 31 - 1) + 1, ld=2 ** 40, out_ld=2 ** 40) == -3
    assert run(cols_=0) == 0
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())                                 # nothing was launched
    assert run() == 0
    assert run(lens=(C.c_uint32 * 2)(8, 8)) == 0                       # L = n - 1: the whole range
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


# ---------------------------------------------------------------- 5. the Python surface: hpdi
def test_hpdi_on_float32_int32_and_strided_views(IV, FORMS):
    for kind in ("lognormal", "counts"):
        m = HR.matrix(kind, 257, 70)
        t = torch.tensor(m).cuda()
        one = IV.hpdi(t)
        assert one.shape == (2, 70) and one.dtype == torch.float32 and one.is_cuda
        assert_same(np_(one), HR.hpdi(m, (0.9,)), f"{kind} prob=0.9")
        probs = (0.5, 0.9, 0.95, float(np.nextafter(1.0, 0.0)), 1e-9)
        many = IV.hpdi(t, probs)
        assert many.shape == (5, 2, 70)
        assert_same(np_(many).reshape(10, 70), HR.hpdi(m, probs), f"{kind} five probabilities")
        assert np.array_equal(bits(np_(many[1])), bits(np_(one))) and IV.hpdi(t, [0.9]).shape == (1, 2, 70)
        view = t[::2, 3:40]                                          # strided rows, offset columns
        assert view.stride(0) == 140 and not view.is_contiguous()
        assert_same(np_(IV.hpdi(view, 0.8)), HR.hpdi(m[::2, 3:40], (0.8,)), f"{kind} view")
        assert_same(np_(IV.hpdi(t[:1], 0.9)), np.stack([m[0], m[0]]).astype(np.float32) + 0.0, "one draw")
    assert IV.hpdi(torch.zeros((5, 0), device="cuda")).shape == (2, 0)
    big = torch.zeros((FORMS[2] + 1, 2), device="cuda")
    with pytest.raises(ValueError, match=rf"n <= {FORMS[2]}\b"):
        IV.hpdi(big)
    with pytest.raises(ValueError, match="unit stride"):
        IV.hpdi(torch.zeros((4, 6), device="cuda")[:, ::2])


# ---------------------------------------------------------------- 6. the regression families
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


def mean_rows(family, X, W, b):
    """The matrix d3p_predict_mean_rows writes for these inputs, fetched to the host: (n, rows) numpy float32."""
    import d3p_amd._lib as L
    from d3p_amd import infer_util as U
    n, d = W.shape
    rows = X.shape[0]
    lat = torch.tensor(W if b is None else np.concatenate([W, np.asarray(b).reshape(n, 1)], axis=1)).cuda().contiguous()
    Xt = torch.tensor(X).cuda()
    out = torch.empty((n, rows), device="cuda")
    model = make_model(family, d, b is not None)
    ms = U._model_struct(model, U._family(model), d)
    L.check(L.load().d3p_predict_mean_rows(L.stream_ptr(), C.byref(ms), L.ptr(Xt), rows, L.ptr(lat), lat.shape[1], 0, d if b is not None else -1, n,
                                           L.ptr(out), rows))
    torch.cuda.synchronize()
    return np_(out).copy()


@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("family", MR.FAMILIES)
def test_credible_interval_hpdi(IV, family, intercept):
    """credible_interval(kind="hpdi") equals the comparator applied to the matrix that d3p_predict_mean_rows wrote for the same inputs, by
    value.  There is NO tolerance and no float64 reference of mu here, on purpose: a highest-density interval is not continuous in its
    inputs -- a perturbation of one ulp can move the narrowest window to another place in the column -- so a bound against a float64 mu
    would not hold.  The same call at two slab sizes (300 rows: 128 + 128 + 44, and whole) gives the same bits."""
    n, rows, d = 64, 300, 33
    X, y, W, b = LR.inputs(family, n, rows, d, intercept)
    model, Xt, s = make_model(family, d, intercept), torch.tensor(X).cuda(), samples_of(W, b)
    res = IV.credible_interval(model, s, Xt, torch.tensor(y).cuda(), rows, prob=0.9, kind="hpdi")
    assert sorted(res) == ["lower", "upper"] and all(v.shape == (rows,) and v.dtype == torch.float32 and v.is_cuda for v in res.values())
    got = np.stack([np_(res["lower"]), np_(res["upper"])])
    written = mean_rows(family, X, W, b)
    assert_same(got, HR.hpdi(written, (0.9,)), f"{family} intercept={intercept}")
    assert_same(got, np_(IV.hpdi(torch.tensor(written).cuda(), 0.9)), "and against hpdi of that matrix")
    for slab_bytes in (4 * n * 128, 1):
        part = IV.credible_interval(model, s, Xt, prob=0.9, kind="hpdi", slab_bytes=slab_bytes)
        assert np.array_equal(bits(np.stack([np_(part["lower"]), np_(part["upper"])])), bits(got)), f"slab_bytes={slab_bytes} changes the bits"
    other = IV.credible_interval(model, s, Xt, prob=0.5, kind="hpdi")
    assert_same(np.stack([np_(other["lower"]), np_(other["upper"])]), HR.hpdi(written, (0.5,)), "prob=0.5")
    eq = IV.credible_interval(model, s, Xt, prob=0.9)                    # (kind="hpdi" is not swallowed: the equal-tailed numbers differ)
    assert sorted(eq) == ["lower", "median", "upper"] and not torch.equal(eq["lower"], res["lower"])
    with pytest.raises(ValueError, match="probs cannot be combined"):
        IV.credible_interval(model, s, Xt, probs=(0.1, 0.9), kind="hpdi")
    with pytest.raises(ValueError, match="kind must be one of"):
        IV.credible_interval(model, s, Xt, kind="HPDI")


def _guide_params(model, d):
    from d3p_amd.models import AutoDiagonalNormal
    guide = AutoDiagonalNormal(model)
    params = {k: torch.tensor(v) for k, v in P.logreg_params(guide, d, True, np.random.default_rng(12)).items()}
    params["auto_loc"] = 0.2 * params["auto_loc"]                 # (keeps the Poisson rates moderate)
    return guide, params


def test_posterior_credible_interval_hpdi_draws_the_latents_of_the_moments(IV):
    """posterior_predictive_moments, posterior_predictive_samples and posterior_credible_interval draw the same latents for one key:
    the samples expose them, credible_interval reduces them."""
    from d3p_amd import predictive as PS
    n, rows, d = 30, 70, 4
    for family in MR.FAMILIES:
        X, _, _, _ = LR.inputs(family, 1, rows, d, True, seed=41)
        model = make_model(family, d, True)
        guide, params = _guide_params(model, d)
        Xt, key = torch.tensor(X).cuda(), P.key(77)
        draws = PS.posterior_predictive_samples(key, n, model, (Xt,), guide, params)
        want = IV.credible_interval(model, {"w": draws["w"], "intercept": draws["intercept"]}, Xt, kind="hpdi")
        got = IV.posterior_credible_interval(key, n, model, (Xt,), guide, params, kind="hpdi")
        assert sorted(got) == ["lower", "upper"]
        assert all(np.array_equal(bits(np_(got[k])), bits(np_(want[k]))) for k in ("lower", "upper"))
        written = mean_rows(family, X, np_(draws["w"]).reshape(n, d), np_(draws["intercept"]).reshape(n))
        assert_same(np.stack([np_(got["lower"]), np_(got["upper"])]), HR.hpdi(written, (0.9,)), family)
        other = IV.posterior_credible_interval(P.key(78), n, model, (Xt,), guide, params, kind="hpdi")
        assert not torch.equal(other["lower"], got["lower"])


@pytest.mark.parametrize("family", ["linear", "poisson"])
def test_predictive_intervals_hpdi_equal_the_rule_on_the_sampled_outcomes(IV, family):
    from d3p_amd import predictive as PS
    n, rows, d = 100, 300, 4
    X, _, W, b = LR.inputs(family, n, rows, d, True, seed=61)
    model, Xt, s, key = make_model(family, d, True), torch.tensor(X).cuda(), samples_of(W, b), P.key(5)
    obs = PS.predictive_samples(key, model, s, Xt)
    assert obs.dtype == (torch.float32 if family == "linear" else torch.int32) and obs.shape == (n, rows)
    got = IV.predictive_interval(key, model, s, Xt, prob=0.8, kind="hpdi")
    assert sorted(got) == ["lower", "upper"]
    assert_same(np.stack([np_(got["lower"]), np_(got["upper"])]), HR.hpdi(np_(obs), (0.8,)), f"{family} predictive_interval")
    guide, params = _guide_params(model, d)
    pobs = PS.posterior_predictive_samples(key, n, model, (Xt,), guide, params)["obs"]
    pgot = IV.posterior_predictive_interval(key, n, model, (Xt,), guide, params, kind="hpdi")
    assert_same(np.stack([np_(pgot["lower"]), np_(pgot["upper"])]), HR.hpdi(np_(pobs), (0.9,)), f"{family} posterior_predictive_interval")
    with pytest.raises(ValueError, match=rf"slab_bytes >= {4 * n * rows}\b"):
        IV.predictive_interval(key, model, s, Xt, kind="hpdi", slab_bytes=4 * n * 128)
    with pytest.raises(TypeError, match="credible_interval"):
        IV.predictive_interval(key, make_model("logistic", d, True), s, Xt, kind="hpdi")


def test_latent_summary_hpdi(IV):
    n, d = 257, 33
    rng = np.random.default_rng(8)
    host = (np.exp(rng.normal(size=(n, d + 1))) * 10.0 ** rng.integers(-2, 3, size=d + 1)).astype(np.float32)
    lat = torch.tensor(host).cuda()
    s = {"w": lat[:, :d], "intercept": lat[:, d]}                    # packed views, as the predictive forms return them
    res, eq = IV.latent_summary(s, prob=0.9, interval="hpdi"), IV.latent_summary(s, prob=0.9)
    assert sorted(res) == ["intercept", "w"] and all(sorted(v) == ["lower", "mean", "median", "std", "upper"] for v in res.values())
    assert res["w"]["lower"].shape == (d,) and res["intercept"]["lower"].shape == () and res["w"]["lower"].dtype == torch.float32
    for name, cols in (("w", slice(0, d)), ("intercept", slice(d, d + 1))):
        r = res[name]
        assert_same(np.stack([np_(r["lower"]).reshape(-1), np_(r["upper"]).reshape(-1)]), HR.hpdi(host[:, cols], (0.9,)), name)
        for k in ("median", "mean", "std"):                           # the median still comes from d3p_col_quantiles, the moments from d3p_col_stats
            assert np.array_equal(np_(r[k]).reshape(-1).view(np.uint8), np_(eq[name][k]).reshape(-1).view(np.uint8)), (name, k)
        assert bool((r["lower"] < eq[name]["lower"]).all())          # skewed to the right: the dense part lies to the left
    one = IV.latent_summary({"w": host[:1, :d]}, interval="hpdi")["w"]
    assert np.array_equal(np_(one["lower"]), host[0, :d]) and np.array_equal(np_(one["upper"]), host[0, :d])


def test_the_default_kind_and_interval_give_todays_bits(IV):
    """kind="equal_tailed" and interval="equal_tailed" spelled out, and left out, are the quantile path: the bits of `quantiles` on the
    matrix the mean kernel wrote, and of np.quantile on the latents."""
    n, rows, d = 64, 129, 4
    X, _, W, b = LR.inputs("poisson", n, rows, d, True)
    model, Xt, s, key = make_model("poisson", d, True), torch.tensor(X).cuda(), samples_of(W, b), P.key(5)
    three = ((1.0 - 0.9) / 2.0, 0.5, (1.0 + 0.9) / 2.0)
    want = np_(IV.quantiles(torch.tensor(mean_rows("poisson", X, W, b)).cuda(), three))
    for kw in ({}, {"kind": "equal_tailed"}):
        res = IV.credible_interval(model, s, Xt, prob=0.9, **kw)
        assert sorted(res) == ["lower", "median", "upper"]
        assert all(np.array_equal(bits(np_(res[k])), bits(want[i])) for i, k in enumerate(("lower", "median", "upper")))
        q = IV.credible_interval(model, s, Xt, probs=QR.PROBS, **kw)
        assert sorted(q) == ["quantiles"] and q["quantiles"].shape == (len(QR.PROBS), rows)
        pi = IV.predictive_interval(key, model, s, Xt, prob=0.8, **kw)
        assert sorted(pi) == ["lower", "median", "upper"]
    from d3p_amd import predictive as PS
    obs = np_(PS.predictive_samples(key, model, s, Xt))
    pi = IV.predictive_interval(key, model, s, Xt, prob=0.8, kind="equal_tailed")
    assert_same(np.stack([np_(pi[k]) for k in ("lower", "median", "upper")]), QR.quantiles(obs, ((1.0 - 0.8) / 2.0, 0.5, (1.0 + 0.8) / 2.0)), "predictive")
    lat = {"w": torch.tensor(W).cuda()}
    a, c = IV.latent_summary(lat, prob=0.9)["w"], IV.latent_summary(lat, prob=0.9, interval="equal_tailed")["w"]
    assert all(np.array_equal(np_(a[k]).view(np.uint8), np_(c[k]).view(np.uint8)) for k in a)
    ref = np.quantile(W.astype(np.float64), three, axis=0, method="linear").astype(np.float32)
    assert_same(np.stack([np_(a[k]) for k in ("lower", "median", "upper")]), ref, "latent_summary")


# ---------------------------------------------------------------- 7. examples
def _example(name):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ex_hpdi_" + name, os.path.join(root, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["linear_regression", "poisson_regression"])
def test_examples_report_the_interval_kind(IV, capsys, name):
    mod = _example(name)
    base = dict(sigma=0.5, clip_threshold=1.0, num_steps=300, learning_rate=2e-2, batch_size=200, dimensions=4, num_samples=2000, obs_scale=0.5)
    mod.main(argparse.Namespace(intervals=50, interval_kind="hpdi", **base))
    out = capsys.readouterr().out
    m = re.search(r"90% highest-density predictive interval \(2000 rows, 50 draws\): coverage ([\d.]+), mean width ([\d.]+)", out)
    assert m, out
    coverage, width = float(m.group(1)), float(m.group(2))
    assert 0.0 <= coverage <= 1.0 and np.isfinite(width) and width > 0.0
    rows = re.findall(r"w\[(\d)\]: mean (-?[\d.]+), std ([\d.]+), median (-?[\d.]+), 90% hpdi (-?[\d.]+) \.\. (-?[\d.]+)", out)
    assert [r[0] for r in rows] == ["0", "1", "2", "3"]
    assert all(float(r[4]) <= float(r[3]) <= float(r[5]) and float(r[2]) > 0.0 for r in rows)
    mod.main(argparse.Namespace(intervals=50, **base))
    plain = capsys.readouterr().out
    mod.main(argparse.Namespace(intervals=50, interval_kind="equal-tailed", **base))
    spelled = capsys.readouterr().out
    def shape(text):
        return re.sub(r"-?\d+\.\d+", "#", text)                            # (the lines with their numbers masked)
    assert shape(plain) == shape(spelled) and "hpdi" not in plain and "highest-density" not in plain
    assert re.search(r"^90% predictive interval \(2000 rows, 50 draws\): coverage [\d.]+, mean width [\d.]+$", plain, re.M)
    assert len(re.findall(r"^w\[\d\]: mean -?[\d.]+, std [\d.]+, median -?[\d.]+, 5% -?[\d.]+, 95% -?[\d.]+$", plain, re.M)) == 4
    rest = [ln for ln in shape(out).splitlines() if "interval" not in ln and not ln.startswith("w[")]
    assert rest == [ln for ln in shape(plain).splitlines() if "interval" not in ln and not ln.startswith("w[")]   # no other line changed
