"""Credible and predictive intervals (d3p_amd.intervals, d3p_col_quantiles), host side: tests/quantiles_ref.py against numpy.quantile
and on its own properties, the non-finite table, the declared symbols, and every argument check of the module that needs no device."""
import os
import re

import numpy as np
import pytest
import torch

from tests import quantiles_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = QR.PROBS + (0.1, 0.25, 0.6, 0.75, 0.9, 0.999)


@pytest.mark.parametrize("name,m", QR.cases(), ids=[c[0] for c in QR.cases()])
def test_rule_equals_numpy_quantile_on_finite_columns(name, m):
    """numpy.quantile(col.astype(float64), p, method='linear') rounded to float32, equal by value, every probability of the sweep."""
    want = np.quantile(m.astype(np.float64), SWEEP, axis=0, method="linear").astype(np.float32)
    got = QR.quantiles(m, SWEEP)
    assert got.shape == (len(SWEEP), m.shape[1]) and got.dtype == np.float32
    assert QR.same_values(got, want), f"{name}: {QR.first_difference(got, want)}"


def test_rule_equals_numpy_quantile_on_continuous_data_at_many_n():
    rng = np.random.default_rng(5)
    for n in (2, 5, 10, 100, 1025):
        m = rng.normal(size=(n, 40)).astype(np.float32)
        want = np.quantile(m.astype(np.float64), SWEEP, axis=0, method="linear").astype(np.float32)
        assert QR.same_values(QR.quantiles(m, SWEEP), want), n


@pytest.mark.parametrize("name,m", QR.cases(), ids=[c[0] for c in QR.cases()])
def test_monotone_extremes_and_permutation(name, m):
    ps = tuple(sorted(SWEEP))
    got = QR.quantiles(m, ps).astype(np.float64)
    assert np.all(np.diff(got, axis=0) >= 0.0), name + ": not monotone in p"
    ends = QR.quantiles(m, (0.0, 1.0))
    assert np.array_equal(ends[0], m.min(axis=0).astype(np.float32)) and np.array_equal(ends[1], m.max(axis=0).astype(np.float32))
    perm = np.random.default_rng(3).permutation(m.shape[0])
    assert QR.same_values(QR.quantiles(m[perm], ps), got.astype(np.float32)), name + ": depends on the order of the draws"


def test_positions():
    assert QR.positions((0.0, 1.0, 0.5), 4) == [(0, 0.0), (3, 0.0), (1, 0.5)]
    assert QR.positions((0.0, 0.3, 1.0), 1) == [(0, 0.0), (0, 0.0), (0, 0.0)]
    from d3p_amd import intervals as IV
    for n in (1, 2, 3, 100, 895, 896, 65535):
        assert IV.positions(SWEEP, n) == QR.positions(SWEEP, n)
        for lo, g in QR.positions(SWEEP, n):
            assert 0 <= lo < n and 0.0 <= g < 1.0 and (g == 0.0 or lo < n - 1)


@pytest.mark.parametrize("col,lo,g,want", QR.NONFINITE)
def test_non_finite_table(col, lo, g, want):
    got = QR.quantiles_at(np.array(col, np.float32).reshape(-1, 1), [(lo, g)])
    assert got.shape == (1, 1) and QR.same_values(got, np.array([[want]], np.float32)), (col, lo, g, got, want)


def test_a_nan_column_touches_no_other():
    m = QR.matrix("normal", 31, 5)
    clean = QR.quantiles(m, QR.PROBS)
    m2 = m.copy()
    m2[7, 2] = np.nan
    got = QR.quantiles(m2, QR.PROBS)
    assert np.isnan(got[:, 2]).all() and np.array_equal(np.delete(got, 2, axis=1), np.delete(clean, 2, axis=1))


def test_int32_counts_above_2_to_24_round_once():
    m = np.array([[16777217], [16777219], [QR.INT32_MAX]], np.int32)
    got = QR.quantiles(m, (0.0, 0.5, 1.0))
    assert got[0, 0] == np.float32(16777216.0) and got[1, 0] == np.float32(16777220.0) and got[2, 0] == np.float32(2147483648.0)


# ---------------------------------------------------------------- the declared surface
def test_symbols_are_declared_and_exported():
    import d3p_amd
    import d3p_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "d3p_hip.h")).read()
    assert re.search(r"\bint d3p_col_quantiles\(void\* stream, const void\* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t cols, uint32_t Q,", hdr)
    assert re.search(r"\buint32_t d3p_col_quantiles_staged_max\(void\);", hdr) and re.search(r"\bint d3p_predict_mean_rows\(", hdr)
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    assert len(L.SIGNATURES["d3p_col_quantiles"][1]) == 11 and len(L.SIGNATURES["d3p_predict_mean_rows"][1]) == 11
    lib = L.load()
    assert lib.d3p_abi_version() == 9
    S = lib.d3p_col_quantiles_staged_max()
    assert 257 < S < 1500 and 32 * 257 * 4 + 32 * 4 * S <= 144 * 1024 < 32 * 257 * 4 + 32 * 4 * (S + 1)
    assert "intervals" in d3p_amd.__all__ and d3p_amd.intervals.quantiles is not None
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "d3p_col_quantiles" in integration and "d3p_predict_mean_rows" in integration


# ---------------------------------------------------------------- host-side argument checks (no device)
def _models():
    from d3p_amd.models import LinearRegression, LogisticRegression, PoissonRegression
    return LinearRegression(4, obs_scale=0.5), PoissonRegression(4), LogisticRegression(4)


def _args(n=10, rows=20, d=4):
    return {"w": np.zeros((n, d), np.float32)}, np.zeros((rows, d), np.float32)


@pytest.mark.parametrize("prob", [0.0, 1.0, -0.1, 1.5, float("nan"), None, "0.9", True])
def test_bad_prob_is_refused(prob):
    from d3p_amd import intervals as IV
    lin, _, _ = _models()
    s, X = _args()
    with pytest.raises(ValueError, match="prob"):
        IV.credible_interval(lin, s, X, prob=prob)
    with pytest.raises(ValueError, match="prob"):
        IV.predictive_interval(None, lin, s, X, prob=prob)
    with pytest.raises(ValueError, match="prob"):
        IV.latent_summary(s, prob=prob)


def test_bad_probs_are_refused():
    from d3p_amd import intervals as IV
    lin, _, _ = _models()
    s, X = _args()
    for probs, msg in (([0.1] * 9, "1 to 8"), ([], "1 to 8"), ([0.5, 1.01], r"\[0, 1\]"), ([-0.01], r"\[0, 1\]"), ([float("nan")], r"\[0, 1\]")):
        with pytest.raises(ValueError, match=msg):
            IV.credible_interval(lin, s, X, probs=probs)
        with pytest.raises(ValueError, match=msg):
            IV.predictive_interval(None, lin, s, X, probs=probs)
        with pytest.raises(ValueError, match=msg):
            IV.quantiles(torch.zeros((3, 2)), probs)
        with pytest.raises(ValueError, match=msg):
            IV.posterior_credible_interval(None, 5, lin, (X,), _guide(lin), {}, probs=probs)


def _guide(model):
    from d3p_amd.models import AutoDiagonalNormal
    return AutoDiagonalNormal(model)


def test_more_than_65535_draws_are_refused():
    from d3p_amd import intervals as IV
    lin, poi, _ = _models()
    s, X = _args(n=65536, rows=3)
    with pytest.raises(ValueError, match="65535"):
        IV.credible_interval(lin, s, X)
    with pytest.raises(ValueError, match="65535"):
        IV.predictive_interval(None, poi, s, X, slab_bytes=1 << 40)
    with pytest.raises(ValueError, match="65535"):
        IV.posterior_credible_interval(None, 65536, lin, (X,), _guide(lin), {})
    with pytest.raises(ValueError, match="65535"):
        IV.posterior_predictive_interval(None, 65536, lin, (X,), _guide(lin), {}, slab_bytes=1 << 40)
    with pytest.raises(ValueError, match="65535"):
        IV.latent_summary(s)


def test_unsupported_models_are_refused():
    from d3p_amd import intervals as IV
    from d3p_amd.models import GaussianMixtureModel
    s, X = _args()
    for model in (GaussianMixtureModel(), object()):
        for call in (lambda: IV.credible_interval(model, s, X), lambda: IV.predictive_interval(None, model, s, X),
                     lambda: IV.posterior_credible_interval(None, 5, model, (X,), None, {}),
                     lambda: IV.posterior_predictive_interval(None, 5, model, (X,), None, {})):
            with pytest.raises(TypeError, match="unsupported model"):
                call()


def test_logistic_regression_has_no_predictive_interval():
    from d3p_amd import intervals as IV
    _, _, log = _models()
    s, X = _args()
    with pytest.raises(TypeError, match="credible_interval"):
        IV.predictive_interval(None, log, s, X)
    with pytest.raises(TypeError, match="credible_interval"):
        IV.posterior_predictive_interval(None, 5, log, (X,), _guide(log), {})


def test_predictive_matrix_must_fit_slab_bytes():
    """d3p_predict_glm has no row offset, so the predictive forms write the matrix whole: the error names the bytes it needs."""
    from d3p_amd import intervals as IV
    lin, poi, _ = _models()
    s, X = _args(n=10, rows=20)
    for model in (lin, poi):
        with pytest.raises(ValueError, match=r"slab_bytes >= 800\b"):
            IV.predictive_interval(None, model, s, X, slab_bytes=799)
        with pytest.raises(ValueError, match=r"slab_bytes >= 800\b"):
            IV.posterior_predictive_interval(None, 10, model, (X,), _guide(model), {}, slab_bytes=1)
    with pytest.raises(TypeError, match="rng_key"):            # 800 bytes fit: the next check is the key's
        IV.predictive_interval(None, lin, s, X, slab_bytes=800)


@pytest.mark.parametrize("slab_bytes", [0, -1, 1.5, None, True])
def test_bad_slab_bytes_are_refused(slab_bytes):
    from d3p_amd import intervals as IV
    lin, _, _ = _models()
    s, X = _args()
    with pytest.raises(ValueError, match="slab_bytes"):
        IV.credible_interval(lin, s, X, slab_bytes=slab_bytes)
    with pytest.raises(ValueError, match="slab_bytes"):
        IV.predictive_interval(None, lin, s, X, slab_bytes=slab_bytes)


def test_quantiles_refuses_what_is_not_a_device_matrix():
    from d3p_amd import intervals as IV
    for bad in (np.zeros((3, 2), np.float32), torch.zeros((3, 2)), torch.zeros((3,)), torch.zeros((3, 2), dtype=torch.float64)):
        with pytest.raises(ValueError, match="CUDA tensor"):
            IV.quantiles(bad, (0.5,))


def test_data_and_sample_checks_are_the_sibling_modules():
    from d3p_amd import intervals as IV
    lin, _, _ = _models()
    s, X = _args()
    with pytest.raises(ValueError, match="columns"):
        IV.credible_interval(lin, s, np.zeros((20, 5), np.float32))
    with pytest.raises(ValueError, match="'w' is missing"):
        IV.credible_interval(lin, {}, X)
    with pytest.raises(ValueError, match="model_args"):
        IV.credible_interval(lin, s)


def test_slab_boundaries_reuse_the_loo_chunk():
    """rows = 300 at 128 rows per slab: 128 / 128 / 44, from infer_util._loo_chunk itself."""
    from d3p_amd import infer_util as U
    n, rows = 100, 300
    chunk = U._loo_chunk(n, 4 * n * 128)
    assert chunk == 128 and U._loo_chunk(n, 1) == 128 and U._loo_chunk(n, 4 * n * 128 + 100) == 128 and U._loo_chunk(n, 4 * n * 256) == 256
    assert [min(chunk, rows - lo) for lo in range(0, rows, chunk)] == [128, 128, 44]
    assert U._loo_chunk(n, 64 << 20) == (64 << 20) // (4 * n) // 128 * 128
