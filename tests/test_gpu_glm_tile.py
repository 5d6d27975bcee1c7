"""One draws x rows product tile (d3p_amd/csrc/d3p_glm_tile.h), several consumers: what two of them compute from the same t[s, r] must
agree bit for bit, and a draw must give the same t in whichever slot of the tile it lies.  Through the C entries, at sizes that end
inside a K slice (32), a half-wave (32) and a row tile (128), for the three families, with and without an intercept."""
import ctypes as C

import numpy as np
import pytest
import torch

from d3p_amd import _lib as L

pytestmark = pytest.mark.gpu

FAMILIES = {"logistic": L.D3P_FAMILY_LOGREG, "linear": L.D3P_FAMILY_LINREG, "poisson": L.D3P_FAMILY_POISSON}
SIGMA = 0.5
DS, ROWS = (1, 33, 65), (1, 65, 129)


def _struct(family, d, intercept):
    return L.LogregModel(d, int(intercept), 1.0, 1.0, 1.0, 1.0, FAMILIES[family], L.D3P_GUIDE_SOFTPLUS, SIGMA)


def _problem(family, d, rows, intercept, seed):
    """X, labels and ONE latent row (weights, then the intercept when there is one); |t| stays below about 4."""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((rows, d)) / np.sqrt(d)).astype(np.float32)
    lat = rng.standard_normal((1, d + int(intercept))).astype(np.float32)
    if family == "logistic":
        y = (rng.random(rows) < 0.5).astype(np.float32)
    elif family == "linear":
        y = rng.standard_normal(rows).astype(np.float32)
    else:
        y = rng.poisson(1.0, rows).astype(np.float32)
    return torch.tensor(X).cuda(), torch.tensor(y).cuda(), torch.tensor(lat).cuda()


def _bits(t):
    return t.view(torch.int32)


def _loglik(fn, ms, X, y, lat, n, out):
    rows, d = X.shape
    L.check(fn(L.stream_ptr(), C.byref(ms), L.ptr(X), L.ptr(y), rows, L.ptr(lat), lat.shape[1], 0, d if ms.intercept else -1, n, L.ptr(out)))
    return out


def _moments(ms, X, lat, n):
    rows, d = X.shape
    mean, var = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    L.check(L.load().d3p_predict_moments(L.stream_ptr(), C.byref(ms), L.ptr(X), rows, L.ptr(lat), lat.shape[1], 0, d if ms.intercept else -1, n,
                                         L.ptr(mean), L.ptr(var)))
    return mean, var


@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_one_draw_lppd_is_the_rows_forms_row(gpu, family, intercept):
    """n = 1: logsumexp over one draw, minus log 1 -- (float)((double) m + log 1 - log 1) is m."""
    lib = L.load()
    for d in DS:
        for rows in ROWS:
            X, y, lat = _problem(family, d, rows, intercept, seed=100 * d + rows)
            ms = _struct(family, d, intercept)
            ll = _loglik(lib.d3p_loglik_rows, ms, X, y, lat, 1, torch.empty((1, rows), device="cuda"))
            lppd = _loglik(lib.d3p_loglik_lppd, ms, X, y, lat, 1, torch.empty(rows, device="cuda"))
            assert bool(torch.isfinite(ll).all()), (d, rows)
            assert torch.equal(_bits(lppd), _bits(ll[0])), (d, rows)


@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_moments_of_identical_draws_are_the_single_draws(gpu, family, intercept):
    """n copies of one draw fill every draw slot of the tile (both wave halves, both 32-draw halves of a wave, a second and a third
    draw tile): the mean's bits are those of the draw alone; the linear family's variance is float32(sigma^2) bit for bit."""
    sig2 = np.float32(np.float64(np.float32(SIGMA)) ** 2)
    for d in DS:
        for rows in ROWS:
            X, _, lat = _problem(family, d, rows, intercept, seed=100 * d + rows + 7)
            ms = _struct(family, d, intercept)
            mean1, var1 = _moments(ms, X, lat, 1)
            assert bool(torch.isfinite(mean1).all()), (d, rows)
            if family == "linear":
                assert np.all(var1.cpu().numpy() == sig2), (d, rows)
            for n in (64, 65, 129, 257):
                mean, var = _moments(ms, X, lat.repeat(n, 1).contiguous(), n)
                assert torch.equal(_bits(mean), _bits(mean1)), (d, rows, n)
                if family == "linear":
                    assert np.all(var.cpu().numpy() == sig2), (d, rows, n)


@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_three_users_of_the_link_agree_bit_for_bit(gpu, family, intercept):
    """glm_mean (d3p_glm_tile.h) is ONE link: for one draw in a padded latent row, d3p_predict_moments' mean (its float64 sums of one
    value round back to the float32 mu) is row 0 of d3p_predict_mean_rows' matrix, and d3p_predict_discrepancy's out[2] at shift 0 is
    the float64 sum of that row in the stated order (tests/discrepancy_ref.py)."""
    from . import discrepancy_ref as R
    lib = L.load()
    d, rows, n = 33, 129, 1
    X, y, w = _problem(family, d, rows, intercept, seed=4242 + int(intercept))
    ld, w_off, b_col = d + 3, 2, (0 if intercept else -1)
    lat = torch.full((n, ld), 7.0, device="cuda")           # (the padding is never read: 7 would show)
    lat[:, w_off:w_off + d] = w[:, :d]
    if intercept:
        lat[:, b_col] = w[:, d]
    ms = _struct(family, d, intercept)
    mu = torch.empty((n, rows), device="cuda")
    L.check(lib.d3p_predict_mean_rows(L.stream_ptr(), C.byref(ms), L.ptr(X), rows, L.ptr(lat), ld, w_off, b_col, n, L.ptr(mu), rows))
    mean, var = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    L.check(lib.d3p_predict_moments(L.stream_ptr(), C.byref(ms), L.ptr(X), rows, L.ptr(lat), ld, w_off, b_col, n, L.ptr(mean), L.ptr(var)))
    assert bool(torch.isfinite(mu).all())
    assert torch.equal(_bits(mean), _bits(mu[0]))
    keys = torch.tensor([[0x9E3779B9 - 2 ** 32, 0x243F6A88]], dtype=torch.int32, device="cuda")
    out = torch.empty((6, n), dtype=torch.float64, device="cuda")
    nbytes = lib.d3p_predict_discrepancy_workspace(rows, n)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    L.check(lib.d3p_predict_discrepancy(L.stream_ptr(), C.byref(ms), L.ptr(X), L.ptr(y), rows, d, L.ptr(lat), ld, w_off, b_col, n, L.ptr(keys), 0.0,
                                        L.ptr(out), L.ptr(ws), nbytes))
    want = R.ordered_sum(mu.cpu().numpy().astype(np.float64))
    assert np.array_equal(out[2].cpu().numpy().view(np.int64), want.view(np.int64)), (out[2], want)
