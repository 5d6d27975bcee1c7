"""Highest-density intervals (d3p_amd.intervals.hpdi, d3p_col_hpdi), host side: the two restatements of the rule in tests/hpdi_ref.py
against each other and against hand-computed columns, the properties of the interval, the window length at its edges, the declared
symbols, and every argument check of the module that needs no device."""
import os
import re

import numpy as np
import pytest
import torch

from tests import hpdi_ref as HR
from tests import quantiles_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    return [(f"{kind} n={n}", HR.matrix(kind, n, 9)) for kind in HR.KINDS for n in HR.HOST_N]


@pytest.mark.parametrize("name,m", _cases(), ids=[c[0] for c in _cases()])
def test_the_two_restatements_agree(name, m):
    lens = HR.sweep_lengths(m.shape[0])
    a, b = HR.hpdi_at(m, lens), HR.hpdi_loop(m, lens)
    assert a.shape == (2 * len(lens), m.shape[1]) and a.dtype == np.float32
    assert HR.same_values(a, b), f"{name}: {HR.first_difference(a, b)}"


def test_the_two_restatements_agree_with_a_nan_column():
    m = HR.matrix("infinities", 31, 9)
    m[7, 2] = np.nan
    lens = HR.sweep_lengths(31)
    a = HR.hpdi_at(m, lens)
    assert np.isnan(a[:, 2]).all() and not np.isnan(np.delete(a, 2, axis=1)).any()
    assert HR.same_values(a, HR.hpdi_loop(m, lens))
    clean = m.copy()
    clean[7, 2] = 0.0
    assert np.array_equal(np.delete(a, 2, axis=1), np.delete(HR.hpdi_at(clean, lens), 2, axis=1))


@pytest.mark.parametrize("col,L,want", HR.FIXED)
def test_fixed_columns(col, L, want):
    m = np.array(col, np.int32 if isinstance(col[0], int) else np.float32).reshape(-1, 1)
    for rule in (HR.hpdi_at, HR.hpdi_loop):
        got = rule(m, [L])
        assert got.shape == (2, 1) and HR.same_values(got[:, 0], np.array(want, np.float32)), (col, L, got, want)
    got = HR.hpdi_at(m, [L])
    assert not np.signbit(got[got == 0.0]).any()                    # a zero end is +0


def test_the_infinite_column_takes_the_first_window_at_every_length():
    m = np.array(HR.INF_COLUMN, np.float32).reshape(-1, 1)
    for L, want in HR.INF_TABLE:
        assert int(HR.first_minimum(m, L)[0]) == 0
        for rule in (HR.hpdi_at, HR.hpdi_loop):
            assert HR.same_values(rule(m, [L])[:, 0], np.array(want, np.float32)), (L, want)


@pytest.mark.parametrize("n", [31, 128, 257, 1025])
def test_exactly_two_windows_tie_and_the_first_wins(n):
    L0, a1, a2 = HR.two_windows_plan(n)
    m = HR.matrix("two_windows", n, 5)
    s = np.sort(m, axis=0)
    lens = s[L0:] - s[:n - L0]
    assert lens.dtype == np.float32
    for c in range(5):
        assert np.flatnonzero(lens[:, c] == lens[:, c].min()).tolist() == [a1, a2]
    assert np.all(HR.first_minimum(m, L0) == a1)
    got = HR.hpdi_at(m, [L0])
    assert np.array_equal(got[0], s[a1]) and np.array_equal(got[1], s[a1 + L0])
    assert HR.two_windows_plan(9) is None and HR.two_windows_plan(3) is None


@pytest.mark.parametrize("name,m", _cases(), ids=[c[0] for c in _cases()])
def test_the_interval_holds_enough_draws_and_no_window_is_narrower(name, m):
    n, cols = m.shape[0], np.arange(m.shape[1])
    exact = m.astype(np.int64) if m.dtype == np.int32 else m + np.float32(0.0)      # (int64 | float32: the lengths' own arithmetic)
    s = np.sort(exact, axis=0)
    for L in HR.sweep_lengths(n):
        i = HR.first_minimum(m, L)
        lower, upper = s[i, cols], s[i + L, cols]
        assert HR.same_values(HR.hpdi_at(m, [L]), np.stack([lower, upper]).astype(np.float32))
        inside = ((exact >= lower) & (exact <= upper)).sum(axis=0)
        assert np.all(inside >= L + 1), f"{name} L={L}: fewer than L + 1 draws inside"
        with np.errstate(invalid="ignore"):
            width, others = upper - lower, s[L:] - s[:n - L]
        assert width.dtype == others.dtype == s.dtype
        ok = np.isnan(width) | np.all(width[None, :] <= others, axis=0)
        assert np.all(ok), f"{name} L={L}: a narrower window exists"


def test_lognormal_draws_pull_the_lower_end_below_the_equal_tailed_one():
    for n in (257, 1025):
        m = HR.matrix("lognormal", n, 40)
        lower, upper = HR.hpdi(m, (0.9,))
        q = QR.quantiles(m, (0.05, 0.95))
        assert np.all(lower < q[0]) and np.all(upper < q[1])
        assert np.all(upper - lower < q[1] - q[0])


def test_window_length_at_the_edges():
    from d3p_amd import intervals as IV
    import d3p_amd._lib as L
    most = int(L.load().d3p_col_hpdi_max_n())
    assert IV.hpdi_max_draws() == most
    below_one = float(np.nextafter(1.0, 0.0))
    assert IV.window_lengths((0.9, 0.5, below_one, 1e-300), 1) == [0, 0, 0, 0]
    assert IV.window_lengths((below_one,), most) == [most - 1] and IV.window_lengths((0.9,), most) == [int(0.9 * most)]
    for n in (1, 2, 3, 10, 1152, 1153, 4608, 4609, most):
        for p in (1e-300, 0.05, 0.5, 0.9, 0.95, below_one):
            (Lq,) = IV.window_lengths((p,), n)
            assert Lq == int(p * n) == HR.window_lengths((p,), n)[0] and 0 <= Lq <= n - 1
    assert HR.sweep_lengths(1) == [0] and HR.sweep_lengths(2) == [0, 1] and HR.sweep_lengths(10) == [0, 1, 5, 8, 9]


# ---------------------------------------------------------------- the declared surface
def test_symbols_are_declared_and_exported():
    import d3p_amd
    import d3p_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "d3p_hip.h")).read()
    assert re.search(r"\bint d3p_col_hpdi\(void\* stream, const void\* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t cols, uint32_t Q, "
                     r"const uint32_t\* len_host,\s+float\* out_dev, int64_t out_ld\);", hdr)
    assert re.search(r"\buint32_t d3p_col_hpdi_max_n\(void\);", hdr) and re.search(r"\buint32_t d3p_col_hpdi_cols_per_group\(uint32_t n\);", hdr)
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    assert len(L.SIGNATURES["d3p_col_hpdi"][1]) == 10 and L.SIGNATURES["d3p_col_hpdi_max_n"][1] == []
    assert len(L.SIGNATURES["d3p_col_hpdi_cols_per_group"][1]) == 1
    assert any(p.endswith("d3p_hpdi.hip") for p in L._SRC)
    lib = L.load()
    assert lib.d3p_abi_version() == 9
    most = lib.d3p_col_hpdi_max_n()
    cap = 144 * 1024
    assert most == cap // 8 and lib.d3p_col_hpdi_cols_per_group(0) == 0 and lib.d3p_col_hpdi_cols_per_group(most + 1) == 0
    for form, wider in ((32, None), (8, 32), (2, 8)):
        top = cap // (4 * form)
        assert lib.d3p_col_hpdi_cols_per_group(top) == form and 4 * top * form <= cap < 4 * (top + 1) * form
        assert lib.d3p_col_hpdi_cols_per_group(top + 1) == {32: 8, 8: 2, 2: 0}[form]
        if wider:
            assert lib.d3p_col_hpdi_cols_per_group(cap // (4 * wider) + 1) == form
    assert lib.d3p_col_hpdi_cols_per_group(1) == 32
    assert "hpdi" in d3p_amd.intervals.__all__ and d3p_amd.intervals.KINDS == ("equal_tailed", "hpdi")
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"`d3p_col_hpdi`[^\n]*numpyro\.diagnostics\.hpdi", integration)


# ---------------------------------------------------------------- host-side argument checks (no device)
def _models():
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    return LinearRegression(4, obs_scale=0.5), PoissonRegression(4), LogisticRegression(4)


def _args(n=10, rows=20, d=4):
    return {"w": np.zeros((n, d), np.float32)}, np.zeros((rows, d), np.float32)


def _guide(model):
    from d3p_amd.models import AutoDiagonalNormal
    return AutoDiagonalNormal(model)


def _calls(IV, model, s, X, n, **kw):
    return (lambda: IV.credible_interval(model, s, X, **kw), lambda: IV.predictive_interval(None, model, s, X, **kw),
            lambda: IV.posterior_credible_interval(None, n, model, (X,), _guide(model), {}, **kw),
            lambda: IV.posterior_predictive_interval(None, n, model, (X,), _guide(model), {}, **kw))


@pytest.mark.parametrize("kind", ["HPDI", "hpd", "", None, 1, "equal-tailed"])
def test_an_unknown_kind_is_refused_and_not_swallowed(kind):
    from d3p_amd import intervals as IV
    lin, _, _ = _models()
    s, X = _args()
    for call in _calls(IV, lin, s, X, 5, kind=kind):
        with pytest.raises(ValueError, match="kind must be one of"):
            call()
    with pytest.raises(ValueError, match="interval must be one of"):
        IV.latent_summary(s, interval=kind)


def test_probs_with_hpdi_is_refused():
    from d3p_amd import intervals as IV
    lin, _, _ = _models()
    s, X = _args()
    for call in _calls(IV, lin, s, X, 5, kind="hpdi", probs=(0.05, 0.95)):
        with pytest.raises(ValueError, match="probs cannot be combined"):
            call()


@pytest.mark.parametrize("prob", [0.0, 1.0, -0.1, 1.5, float("nan"), None, "0.9", True])
def test_bad_prob_is_refused_for_hpdi(prob):
    from d3p_amd import intervals as IV
    lin, _, _ = _models()
    s, X = _args()
    for call in _calls(IV, lin, s, X, 5, kind="hpdi", prob=prob):
        with pytest.raises(ValueError, match="prob"):
            call()
    with pytest.raises(ValueError, match="prob"):
        IV.latent_summary(s, prob=prob, interval="hpdi")
    with pytest.raises(ValueError, match="prob"):
        IV.hpdi(torch.zeros((3, 2)), prob)


def test_hpdi_refuses_bad_probability_sequences_and_what_is_not_a_device_matrix():
    from d3p_amd import intervals as IV
    for probs, msg in (([0.1] * 9, "1 to 8"), ([], "1 to 8"), ([0.5, 1.0], "prob"), ([0.0], "prob"), ([float("nan")], "prob")):
        with pytest.raises(ValueError, match=msg):
            IV.hpdi(torch.zeros((3, 2)), probs)
    for bad in (np.zeros((3, 2), np.float32), torch.zeros((3, 2)), torch.zeros((3,)), torch.zeros((3, 2), dtype=torch.float64)):
        with pytest.raises(ValueError, match="CUDA tensor"):
            IV.hpdi(bad, 0.9)
        with pytest.raises(ValueError, match="CUDA tensor"):
            IV.hpdi(bad, (0.5, 0.9))


def test_more_draws_than_the_sort_holds_are_refused_with_the_maximum():
    from d3p_amd import intervals as IV
    most = IV.hpdi_max_draws()
    lin, poi, _ = _models()
    s, X = _args(n=most + 1, rows=3)
    for call in _calls(IV, lin, s, X, most + 1, kind="hpdi", slab_bytes=1 << 40):
        with pytest.raises(ValueError, match=rf"n <= {most}\b"):
            call()
    with pytest.raises(ValueError, match=rf"n <= {most}\b"):
        IV.latent_summary(s, interval="hpdi")
    with pytest.raises(TypeError, match="rng_key"):                 # the equal-tailed kind still runs this many draws: the next check is the key's
        IV.predictive_interval(None, poi, s, X, slab_bytes=1 << 40)


def test_family_guide_and_slab_refusals_are_unchanged_with_hpdi():
    from d3p_amd import intervals as IV
    from d3p_amd.models import GaussianMixtureModel
    lin, poi, log = _models()
    s, X = _args()
    for model in (GaussianMixtureModel(), object()):
        for call in (lambda: IV.credible_interval(model, s, X, kind="hpdi"), lambda: IV.predictive_interval(None, model, s, X, kind="hpdi"),
                     lambda: IV.posterior_credible_interval(None, 5, model, (X,), None, {}, kind="hpdi"),
                     lambda: IV.posterior_predictive_interval(None, 5, model, (X,), None, {}, kind="hpdi")):
            with pytest.raises(TypeError, match="unsupported model"):
                call()
    with pytest.raises(TypeError, match="credible_interval"):
        IV.predictive_interval(None, log, s, X, kind="hpdi")
    with pytest.raises(TypeError, match="credible_interval"):
        IV.posterior_predictive_interval(None, 5, log, (X,), _guide(log), {}, kind="hpdi")
    for model in (lin, poi):
        with pytest.raises(ValueError, match=r"slab_bytes >= 800\b"):
            IV.predictive_interval(None, model, s, X, slab_bytes=799, kind="hpdi")
        with pytest.raises(ValueError, match=r"slab_bytes >= 800\b"):
            IV.posterior_predictive_interval(None, 10, model, (X,), _guide(model), {}, slab_bytes=1, kind="hpdi")
    for slab_bytes in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError, match="slab_bytes"):
            IV.credible_interval(lin, s, X, slab_bytes=slab_bytes, kind="hpdi")
    with pytest.raises(TypeError, match="rng_key"):                 # every host check passed: the next one is the key's
        IV.predictive_interval(None, lin, s, X, slab_bytes=800, kind="hpdi")


def test_the_examples_take_the_interval_kind():
    for name in ("linear_regression", "poisson_regression"):
        src = open(os.path.join(ROOT, "examples", name + ".py")).read()
        assert "--interval-kind" in src and "choices=('equal-tailed', 'hpdi')" in src and "default='equal-tailed'" in src
