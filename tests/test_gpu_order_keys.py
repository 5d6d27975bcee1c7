"""The one order-key map of d3p_amd/csrc/d3p_colreduce.h on the GPU, through every reducer that selects or sorts on it: a column of
the values at which an order-preserving image of a float32 (an int32) can go wrong -- the infinities, the largest finite values, the
smallest denormals, both zeros -- against np.sort of the same values in float64.  Every position is exact (g = 0, one window), so the
outputs are stored values and are compared BY VALUE (-0 equal to +0), never within a tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = np.float32(2.0 ** -149)
SPECIALS = np.array([-np.inf, -FLT_MAX, -1.0, -DENORM_MIN, -0.0, 0.0, DENORM_MIN, 1.0, FLT_MAX, np.inf], np.float32)
INTS = np.array([np.iinfo(np.int32).min, -1, 0, 1, np.iinfo(np.int32).max], np.int32)


@pytest.fixture(scope="module")
def IV(gpu):
    from d3p_amd import intervals
    return intervals


def shuffled(values, n, cols, seed):
    """(n, cols): the values tiled to n rows, every column in an order of its own."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(np.resize(values, n)) for _ in range(cols)], axis=1)


def expected_sorted(m):
    """np.sort of every column in float64; no NaN, so that no comparison below is skipped."""
    e = np.sort(m.astype(np.float64), axis=0)
    assert not np.isnan(e).any()
    return e


def exact_probs(IV, n):
    """k / (n - 1), k = 0 .. n - 1: the positions are (k, 0), the results the order statistics themselves."""
    probs = [k / (n - 1) for k in range(n)]
    assert IV.positions(probs, n) == [(k, 0.0) for k in range(n)]
    return probs


def order_statistics(IV, m):
    """All n order statistics of every column through IV.quantiles, at most 8 probabilities per call."""
    n = m.shape[0]
    probs = exact_probs(IV, n)
    dev = torch.tensor(m).cuda()
    return np.concatenate([IV.quantiles(dev, probs[k:k + IV.MAX_PROBS]).cpu().numpy() for k in range(0, n, IV.MAX_PROBS)])


def whole_window_prob(IV, n):
    prob = (n - 0.5) / n
    assert IV.window_lengths((prob,), n) == [n - 1]
    return prob


def test_quantiles_order_the_special_values(IV):
    m = shuffled(SPECIALS, 10, 33, 0)                       # 33 columns: a second 32-column group
    assert np.array_equal(order_statistics(IV, m).astype(np.float64), expected_sorted(m))


@pytest.mark.parametrize("n,cols", [(10, 33), (1153, 9)])   # the 32-column form and, one draw above its limit, the 8-column form
def test_hpdi_whole_window_ends_at_the_extremes(IV, n, cols):
    import d3p_amd._lib as L
    assert L.load().d3p_col_hpdi_cols_per_group(n) == (32 if n == 10 else 8)
    m = shuffled(SPECIALS, n, cols, 1)
    e = expected_sorted(m)
    out = IV.hpdi(torch.tensor(m).cuda(), whole_window_prob(IV, n)).cpu().numpy()
    assert out.shape == (2, cols)
    assert np.array_equal(out[0].astype(np.float64), e[0]) and np.array_equal(out[1].astype(np.float64), e[-1])


def test_norm_profile_orders_the_finite_non_negative_values(gpu):
    from d3p_amd import clipping as CL
    values = SPECIALS[np.isfinite(SPECIALS) & (SPECIALS >= 0)]              # -0, +0, the denormal, 1, FLT_MAX
    assert len(values) == 5
    e = expected_sorted(values[:, None])[:, 0]
    norms = np.random.default_rng(2).permutation(values)
    probs = [k / 4 for k in range(5)]
    prof = CL.norm_profile(torch.tensor(norms).cuda(), (), probs)
    assert prof.n == 5 and prof.n_nonfinite == 0
    assert np.array_equal(np.array(prof.quantiles, np.float64), e) and prof.max == e[-1]


def test_int32_keys_order_the_extremes(IV):
    m = shuffled(INTS, 5, 33, 3)
    e = expected_sorted(m).astype(np.float32)               # the outputs are float32: INT32_MAX rounds to 2^31, once
    assert np.array_equal(order_statistics(IV, m), e)
    out = IV.hpdi(torch.tensor(m).cuda(), whole_window_prob(IV, 5)).cpu().numpy()
    assert np.array_equal(out[0], e[0]) and np.array_equal(out[1], e[-1])
