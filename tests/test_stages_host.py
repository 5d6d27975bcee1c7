"""tests/stages_ref.py pinned on the CPU, so that the comparator of tests/test_gpu_stages.py is not its own witness: the reference's
known answers quoted elsewhere in this repository, scipy / numpy / hand computations of the same formulas, the non-finite
conventions, the oracle's mixture log-prob on the rows where it used to return NaN, and the conditions the GPU assertions rely on
(decision margins, which rows overflow, the complete case lists)."""
import math

import numpy as np
import pytest
from scipy.special import logsumexp
from scipy.stats import norm

from . import stages_ref as S

U = S.U


# ------------------------------------------------------------------------------------------------------------ known answers
def test_full_norm_known_answers_and_every_order():
    ones = np.ones(17 * 2 * 3 + 2 * 54 + 2 * 3 + 3 * 4 * 5, np.float32)           # the reference's all-ones tree: 276 elements
    assert abs(S.full_norm(ones)[0] - 16.613247) < 1e-6
    assert S.full_norm(np.zeros(0, np.float32)) == (0.0, 0.0)
    v = S.norm_inputs(257, "zeros")[0]
    a = np.abs(v.astype(np.float64))
    want = {0: float((v != 0).sum()), 1: a.sum(), 2: math.sqrt((a * a).sum()), 3: (a ** 3).sum() ** (1 / 3),
            0.5: (a[a > 0] ** 0.5).sum() ** 2, math.inf: a.max(), -math.inf: a.min()}
    for order, w in want.items():
        got = S.full_norm(v, order)[0]
        assert got == np.linalg.norm(v.astype(np.float64), ord=order)
        assert abs(got - w) <= 1e-12 * abs(w), order
    assert S.full_norm(v, -1.5)[0] == 0.0                        # a zero entry: 0^-1.5 = inf, inf^(-1/1.5) = 0, as numpy
    assert set(S.NORM_ORDS) == set(want) | {-1.5}


def test_clip_known_answer_and_conventions():
    g = np.zeros((2, 12), np.float32)
    g[0, :10] = 1.0
    g[1, 10:] = 1.0                                              # norms sqrt(10), sqrt(2) -> 2, sqrt(2) at c = 2
    out, _ = S.clip_rows(g, 2.0)
    assert np.allclose(np.sqrt((out * out).sum(axis=1)), [2.0, math.sqrt(2.0)], rtol=1e-15)
    assert np.array_equal(out[1], g[1].astype(np.float64))
    with pytest.raises(ValueError):
        S.clip_rows(g, 0.0)
    assert np.array_equal(S.clip_rows(g, math.inf)[0], g.astype(np.float64))
    h = np.array([[3.0, np.nan, 1.0], [3.0, np.inf, 1.0], [1e20, -1e20, 1e20], [0.0, 0.0, 0.0]], np.float32)
    out, _ = S.clip_rows(h, 1.0)
    assert np.isnan(out[0]).all()
    assert out[1, 0] == 0.0 and np.isnan(out[1, 1]) and out[1, 2] == 0.0
    assert np.array_equal(out[2], [0.0, -0.0, 0.0]) and np.array_equal(out[3], [0.0, 0.0, 0.0])


def test_combine_and_perturb_apply_by_hand():
    g = np.array([[1.0, -2.0], [3.0, 2.0], [5.0, np.nan]], np.float32)
    avg, cond, loss, lcond = S.combine(g, np.array([1.0, -2.0, 4.0], np.float32))
    assert avg[0] == 3.0 and cond[0] == 3.0 and np.isnan(avg[1]) and loss == 1.0 and lcond == 7.0 / 3.0
    assert S.combine(g)[2:] == (None, None)
    val, cond = S.perturb_apply(np.array([1.0], np.float32), np.array([-2.0], np.float32), 1.5, 2.0, 8.0, 0.5, 4.0)
    assert val[0] == (1.0 - 2.0 * 1.5 * 0.25) * 2.0 and cond[0] == (1.0 + 0.75) * 2.0


def test_adam_three_steps_by_hand_and_conventions():
    lr, b1, b2, eps = (float(np.float32(h)) for h in S.ADAM_HYPER[0])
    x, m, v = 0.25, 0.0, 0.0
    X, M, V = (np.array([t], np.float32) for t in (x, m, v))
    for i, g in enumerate((0.5, -0.125, 2.0)):
        m = (1 - b1) * g + b1 * m
        v = (1 - b2) * g * g + b2 * v
        x = x - lr * (m / (1 - b1 ** (i + 1))) / (math.sqrt(v / (1 - b2 ** (i + 1))) + eps)
        r = S.adam(X, M, V, np.array([g], np.float32), i, *S.ADAM_HYPER[0])
        assert abs(r["x"][0] - x) < 1e-15 and abs(r["m"][0] - m) < 1e-17 and abs(r["v"][0] - v) < 1e-17
        X, M, V = (np.array([t], np.float32) for t in (x, m, v))
        x, m, v = float(X[0]), float(M[0]), float(V[0])
    # g * g beyond float32: v = +inf and x stays; 1e19 squares to 1e38, inside
    r = S.adam(np.array([1.0, 1.0], np.float32), np.zeros(2, np.float32), np.full(2, 0.5, np.float32),
               np.array([1e20, 1e19], np.float32), 999)
    assert r["v"][0] == math.inf and r["x"][0] == 1.0 and np.isfinite(r["v"][1]) and r["x"][1] < 1.0
    assert float(np.float32(1e20)) ** 2 > S.F32_OVERFLOW and float(np.float32(1e19)) ** 2 < S.F32_OVERFLOW / 2
    val, cond = S.sgd(np.array([1.0], np.float32), np.array([-4.0], np.float32), 0.25)
    assert val[0] == 2.0 and cond[0] == 2.0
    # step 1: the square of the float32 decay rate is not a float32, which is what adam_pow_eps(1) accounts for
    for _, hb1, hb2, _ in S.ADAM_HYPER:
        for b in (hb1, hb2):
            sq = float(np.float32(b)) ** 2
            assert float(np.float32(sq)) != sq and abs(float(np.float32(sq)) - sq) <= U * sq
    assert S.adam_pow_eps(0) == 0.0 and S.adam_pow_eps(10 ** 6) == 0.0 and S.adam_pow_eps(9) == S.adam_pow_eps(999) == S.POWF_REL
    assert float(np.float32(0.999)) ** (10 ** 6 + 1) == 0.0


def test_adadp_known_answers():
    """tests/test_adadp_optimizer.py:66-131 on the flat vector of the reference's template (86 elements)."""
    P = 7 * 10 + 7 + 2 * 7 + 2
    full = lambda t: np.full(P, t, np.float32)
    r = S.adadp(full(0.0), 1.0, full(0.0), full(0.0), full(1.0), 0)
    assert np.array_equal(r["x"], full(-0.5)) and np.array_equal(r["x_stepped"], full(-1.0)) and r["lr"] == 1.0
    r = S.adadp(full(-0.5), 1.0, full(-1.0), full(0.0), full(2.0), 1, tol=5.0, stability_check=False)
    assert np.array_equal(r["x"], full(-1.5)) and abs(r["lr"] - 1.018308251) < 1e-8 and not r["reject"]
    r = S.adadp(full(-0.5), 1.0, full(-1.0), full(0.0), full(3.0), 1, tol=5.0, stability_check=True)
    assert np.array_equal(r["x"], full(0.0)) and r["reject"] and r["lr"] == float(np.float32(0.9))
    r = S.adadp(full(2.0), 0.5, full(2.0), full(2.0), full(0.0), 1)
    assert r["err"] == 0.0 and r["lr"] == 0.5 * float(np.float32(1.1)) and not r["reject"]
    # max(1, x) without the absolute value: x_stepped = -4 divides by 1, x_stepped = 4 by 4
    r = S.adadp(np.array([0.0, 0.0], np.float32), 1.0, np.array([-4.0, 4.0], np.float32), np.zeros(2, np.float32),
                np.zeros(2, np.float32), 1, tol=100.0)
    assert abs(r["err"] - math.sqrt(16.0 + 1.0)) < 1e-15


def test_gmm_log_prob_against_scipy_and_the_non_finite_conventions():
    for K, d, B in [(3, 2, 2), (5, 65, 4), (17, 7, 3)]:
        x, locs, scales, pis = S.gmm_input(K, d, B)
        with np.errstate(divide="ignore"):
            comp = np.stack([norm(locs[k].astype(np.float64), scales[k].astype(np.float64)).logpdf(x.astype(np.float64)).sum(axis=-1)
                             for k in range(K)]) + np.log(pis.astype(np.float64))[:, None]
        want = logsumexp(comp, axis=0)
        got = S.gmm_log_prob(x, locs, scales, pis)[0]
        assert np.isfinite(want).all() and np.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert np.array_equal(S.logsumexp_rows([[-np.inf, -np.inf], [np.nan, 0.0], [-np.inf, 0.0], [-np.inf, np.nan]]),
                          [-np.inf, np.nan, 0.0, np.nan], equal_nan=True)
    x, locs, scales, pis = S.gmm_input(5, 3, 4)
    x[0, 1] = np.inf
    x[1, :] = 1e30                           # finite, but z * z leaves float32 (and not float64)
    x[2, 2] = np.nan
    got = S.gmm_log_prob(x, locs, scales, pis)[0]
    assert got[0] == -np.inf and got[1] == -np.inf and np.isnan(got[2]) and np.isfinite(got[3])
    z = (np.float64(1e30) - locs.astype(np.float64)) / scales.astype(np.float64)
    assert (z * z > S.F32_OVERFLOW).all() and np.isfinite(z * z).all()


def test_oracle_mixture_log_prob_gives_minus_inf_where_every_component_is(O):
    """A row with an infinite coordinate makes every component -inf: the oracle's logsumexp must give -inf like the restatement (and
    jax's), not -inf - -inf = NaN; the finite neighbours keep their values."""
    for K, d, B in [(1, 1, 1), (4, 63, 5), (17, 65, 4)]:
        x, locs, scales, pis = S.gmm_input(K, d, B)
        clean = O.gmm_log_prob(x, locs, scales, pis)
        for rotation in range(3):
            xh, placed = S.gmm_hostile(x, rotation)
            got, want = O.gmm_log_prob(xh, locs, scales, pis), S.gmm_log_prob(xh, locs, scales, pis)[0]
            for row in range(B):
                if row in placed:
                    assert np.array_equal(got[row], np.float32(want[row]), equal_nan=True), (K, d, B, row, placed[row], got[row])
                else:
                    assert got[row] == clean[row]
            assert np.allclose(clean, S.gmm_log_prob(x, locs, scales, pis)[0], rtol=S.GMM_RTOL, atol=S.GMM_ATOL)


def test_tf_randint_restatement_against_the_oracle(O):
    """Python integers with the two uint32 wraps written out against the oracle's C, fed the same split keys and word streams."""
    for lo, hi in S.RANDINT_RANGES:
        for n in S.RANDINT_N:
            key = [3, 1000 + n]
            k = O.tf_split(key, 2)
            got = S.tf_randint(O.tf_random_words(k[0], n), O.tf_random_words(k[1], n), lo, hi)
            assert np.array_equal(got, O.tf_randint(key, n, lo, hi)), (lo, hi, n)
            assert got.min() >= lo and got.max() < max(hi, lo + 1)
    # the wrapping multiplier is not 2^32 % span: at span 65537 it is 0, at 2^32 - 1 it is 0 too (the high word drops out)
    assert ((65536 % 65537) ** 2 % 2 ** 32) % 65537 == 0 and 2 ** 32 % 65537 == 1
    assert np.array_equal(S.tf_randint([7, 2 ** 32 - 1], [5, 65536], 0, 65537), [5, 65536])


def test_entries_refuse_null_pointers_and_bad_sizes_before_any_launch():
    """Every refusal the host code makes before it launches anything, without a device: null pointers, c == 0, K outside 1 .. 64,
    empty inputs, a workspace below d3p_adadp_workspace()."""
    import ctypes as C
    import d3p_amd._lib as L
    lib = L.load()
    one = C.c_void_p(256)            # a non-null address nothing reads: every call below returns before a launch

    def refused(rc, text, code=-1):
        assert rc == code and text in lib.d3p_last_error(), (rc, lib.d3p_last_error())

    refused(lib.d3p_clip_rows(None, one, 3, 4, 0.0), b"clipping threshold")
    refused(lib.d3p_clip_rows(None, None, 3, 4, 1.0), b"null pointer")
    refused(lib.d3p_full_norm(None, one, 4, None, None, 0), b"null pointer")
    refused(lib.d3p_full_norm(None, None, 4, one, None, 0), b"null pointer")
    refused(lib.d3p_full_norm_ord(None, one, 0, 1.0, one), b"empty vector")
    refused(lib.d3p_full_norm_ord(None, one, 4, float("nan"), one), b"ord is NaN")
    refused(lib.d3p_combine(None, None, None, 3, 4, one, None), b"null pointer")
    refused(lib.d3p_combine(None, one, None, 0, 4, one, None), b"empty input")
    refused(lib.d3p_combine(None, one, None, 3, 0, one, None), b"empty input")
    sizes = (C.c_int32 * 2)(3, -1)
    refused(lib.d3p_perturb(None, one, one, sizes, 2, 1.0, 1.0, one, 1.0, one, None), b"null pointer")
    refused(lib.d3p_perturb(None, one, one, sizes, 0, 1.0, 1.0, one, 1.0, one, one), b"at least one site")
    refused(lib.d3p_perturb_apply(None, one, None, 4, 1.0, 1.0, one, 1.0, one), b"null pointer")
    refused(lib.d3p_perturb_apply(None, one, one, 4, 1.0, 1.0, None, 1.0, one), b"null meta")
    refused(lib.d3p_adam_step(None, one, one, one, None, one, 4, 1e-3, 0.9, 0.999, 1e-8), b"null pointer")
    refused(lib.d3p_sgd_step(None, one, one, None, 4, 0.1), b"null pointer")
    refused(lib.d3p_adadp_step(None, one, one, one, one, one, one, 4, 1.0, 1, None, 260), b"null pointer")
    assert lib.d3p_adadp_workspace() == 65 * 4
    rc = lib.d3p_adadp_step(None, one, one, one, one, one, one, 4, 1.0, 1, one, 259)
    assert rc not in (0, -1) and b"workspace too small" in lib.d3p_last_error()
    refused(lib.d3p_gmm_log_prob(None, one, 2, 3, one, one, None, 2, one), b"null pointer")
    refused(lib.d3p_gmm_log_prob(None, one, 2, 3, one, one, one, 0, one), b"d and K must be >= 1")
    refused(lib.d3p_gmm_log_prob(None, one, 2, 0, one, one, one, 2, one), b"d and K must be >= 1")
    rc = lib.d3p_gmm_log_prob(None, one, 2, 3, one, one, one, 65, one)
    assert rc not in (0, -1) and b"at most 64 mixture components" in lib.d3p_last_error()
    refused(lib.d3p_tf_randint(None, None, 4, 0, 5, one), b"null pointer")


# ------------------------------------------------------------------------------------------------------------ conditions
def test_case_lists_are_complete():
    assert len(S.clip_cases()) == 12 and {p for p, _ in S.clip_cases()} == set(S.CLIP_P) and {b for _, b in S.clip_cases()} == set(S.CLIP_B)
    seen = {S.clip_kind(i, r) for i, (P, B) in enumerate(S.clip_cases()) for r in range(B)}
    assert seen == set(S.CLIP_KINDS)
    for wide in (False, True):               # every kind at a row of one trip of the lane loop and at one of several
        assert {S.clip_kind(i, r) for i, (p, B) in enumerate(S.clip_cases()) if (p > 64) == wide for r in range(B)} == set(S.CLIP_KINDS)
    assert len(S.norm_cases()) == 36 and len(S.NORM_ORDS) == 8
    assert [len(S.norm_inputs(n, "nan")) for n in S.NORM_N] == [1, 2, 2, 3, 4, 4]
    assert len(S.combine_cases()) == 14 and {b for b, _ in S.combine_cases()} == set(S.COMBINE_B) and {p for _, p in S.combine_cases()} == set(S.COMBINE_P)
    assert len(S.adam_cases()) == 30 and len(S.ADAM_HYPER) == 2
    assert len(S.adadp_cases()) == 24
    assert len(S.gmm_cases()) == 14 and {k for k, _, _ in S.gmm_cases()} == set(S.GMM_K)
    assert {d for _, d, _ in S.gmm_cases()} == set(S.GMM_D) and {b for _, _, b in S.gmm_cases()} == set(S.GMM_B)
    assert [S.gmm_hostile_positions(B) for B in S.GMM_B] == [[0], [0, 1, 2], [0, 2, 3], [0, 2, 4], [0, 130, 256]]
    assert len(S.RANDINT_N) * len(S.RANDINT_RANGES) == 10 and S.PERTURB_SITES[0] == [0, 1, 15, 16, 17, 0, 2049]
    specials = {(P, int(s)) for P, i in S.adam_cases() for s in S.adam_input(P, i, False)[4] if s >= 0}
    assert {s for P, s in specials if P == 1} == {0, 1, 2, 3}


@pytest.mark.parametrize("case_index", range(12))
def test_clip_rows_are_what_their_kind_says(case_index):
    g, c = S.clip_input(case_index)
    g64 = g.astype(np.float64)
    with np.errstate(all="ignore"):
        ss = (g64 * g64).sum(axis=1)
        ss32 = (g * g).sum(axis=1, dtype=np.float32)
    for r in range(g.shape[0]):
        kind, n = S.clip_kind(case_index, r), math.sqrt(ss[r]) if np.isfinite(ss[r]) else ss[r]
        if kind == "below":
            assert n < c * (1 - 1e-3)
        elif kind == "above":
            assert n > c * (1 + 1e-3)
        elif kind == "at_c":
            assert c * (1 - 2 * U) <= n <= c * (1 + 2 * U)
        elif kind == "zero":
            assert n == 0.0
        elif kind == "overflow":                  # beyond float32, inside float64
            assert np.isfinite(ss[r]) and ss[r] > 2 * S.F32_OVERFLOW and ss32[r] == np.inf and np.isfinite(g[r]).all()
        elif kind == "nan":
            assert np.isnan(g[r]).sum() == 1
        else:
            assert np.isposinf(g[r]).sum() == 1 and np.isfinite(g[r]).sum() == g.shape[1] - 1
        if kind in ("below", "above", "at_c"):
            assert ss[r] < S.F32_OVERFLOW / 4


@pytest.mark.parametrize("P", S.ADADP_P)
def test_adadp_decisions_cannot_flip_on_rounding(P):
    for scenario in S.ADADP_SCENARIOS:
        x0, g0, g1, tol, check = S.adadp_input(P, scenario)
        even = S.adadp(x0, S.ADADP_LR0, S.f32(np.zeros(P)), x0, g0, 0)
        odd = S.adadp(S.f32(even["x"]), even["lr"], S.f32(even["x_stepped"]), S.f32(even["x_prev"]), g1, 1, tol, check)
        tol32 = float(np.float32(tol))
        if scenario == "zero_grad":
            assert odd["err"] == 0.0 and not odd["reject"] and odd["lr"] == S.ADADP_LR0_F32 * float(np.float32(1.1))
            continue
        assert odd["err"] > 0 and not (tol32 * (1 - 1e-4) <= odd["err"] <= tol32 * (1 + 1e-4))
        assert odd["reject"] == (scenario == "reject") and (odd["err"] > tol32) == (scenario != "accept")
        factor = odd["lr"] / S.ADADP_LR0_F32                  # inside the clamps: the learning rate really moves with the error
        assert 0.9 + 1e-3 < factor < 1.1 - 1e-3 and abs(factor - 1.0) > 1e-2


def test_combine_columns_cancel():
    for B, P in S.combine_cases():
        g, loss = S.combine_input(B, P)
        avg, cond, _, _ = S.combine(g, loss)
        if B >= 8:
            assert (np.abs(avg[::4]) <= 2.0 ** -10 * cond[::4]).all() and (np.abs(avg[::4]) > 0).all()


def test_mixture_cases_hold_what_they_claim():
    for K, d, B in S.gmm_cases():
        x, locs, scales, pis = S.gmm_input(K, d, B)
        assert scales.min() >= 0.2 and scales.max() <= 1.2 and abs(float(pis.astype(np.float64).sum()) - 1) < 1e-6
        if K >= 3:
            assert (pis == 0).sum() == 1
        val = S.gmm_log_prob(x, locs, scales, pis)[0]
        assert np.isfinite(val).all()
        if K >= 2:                              # the far component is >= 10^3 log-units below the best: its exp is 0 in float32
            z = (x.astype(np.float64)[:, None, :] - locs.astype(np.float64)[None]) / scales.astype(np.float64)[None]
            comp = (-0.5 * z * z - np.log(scales.astype(np.float64))[None] - S.HALF_LOG_2PI).sum(axis=2)
            assert (comp[:, :K - 1].max(axis=1) - comp[:, K - 1] > 1e3).all()
        for rotation in range(3):
            xh, placed = S.gmm_hostile(x, rotation)
            want = S.gmm_log_prob(xh, locs, scales, pis)[0]
            for row, kind in placed.items():
                assert np.isnan(want[row]) if kind == "nan" else want[row] == -np.inf
            keep = [r for r in range(B) if r not in placed]
            assert np.array_equal(want[keep], val[keep])
