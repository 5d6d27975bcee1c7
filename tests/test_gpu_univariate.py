"""d3p_sort_columns, d3p_column_cdf_distance and d3p_amd.univariate on the GPU against tests/univariate_ref.py: by value (bit patterns,
integers) everywhere but w1, which is held to the bound derived in the entry's header."""
import math

import numpy as np
import pytest
import torch

import d3p_amd._lib as L
from d3p_amd import covariance as CV
from d3p_amd import univariate as UV
from tests import univariate_ref as UR

pytestmark = pytest.mark.gpu
NEG_NAN, POS_NAN, NEG_INF, POS_INF = 0xffc00001, 0x7fc00000, 0xff800000, 0x7f800000


def _shapes():   # the wave-chunk, tile, block (T) and staging edges, from the query functions (host-only: callable while collecting)
    lib = L.load()
    T, stage = lib.d3p_sort_columns_block_keys(), lib.d3p_sort_columns_staged_keys()
    ns = (1, 2, 63, 64, 65, 1023, 1025, T - 1, T, T + 1, stage + 1, 2 * stage + 3617)
    assert [lib.d3p_sort_columns_rank_stride(n) for n in ns[-3:]] == [1, 2, 3]
    return [(n, 65) for n in ns] + [(T + 1, d) for d in (1, 2, 63, 64)]


def table(n, d, is_int, seed):
    """(n, d) uint32 words, one kind of content per column (kind = column mod the number of kinds)."""
    r = np.random.default_rng(seed)
    ramp = np.arange(n, dtype=np.int64)
    byte = r.integers(0, 256, n).astype(np.uint32)
    if is_int:
        ends = r.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
        ends[r.integers(0, n)], ends[r.integers(0, n)] = -2 ** 31, 2 ** 31 - 1
        kinds = [r.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), r.choice(np.array([-7, 0, 9], np.int32), n, p=[0.01, 0.98, 0.01]),
                 np.full(n, 5, np.int32), (ramp - n // 2).astype(np.int32), (n // 2 - ramp).astype(np.int32), byte << np.uint32(24), byte, ends]
    else:
        normal = r.normal(size=n).astype(np.float32)
        with_inf, with_nan = normal.copy().view(np.uint32), normal.copy().view(np.uint32)
        with_inf[r.integers(0, n)], with_inf[r.integers(0, n)] = NEG_INF, POS_INF
        with_nan[r.integers(0, n)], with_nan[r.integers(0, n)] = NEG_NAN, POS_NAN
        kinds = [normal, r.choice(np.array([-1.5, 0.25, 3.0], np.float32), n, p=[0.01, 0.98, 0.01]), np.full(n, 2.5, np.float32),
                 ramp.astype(np.float32), (-ramp).astype(np.float32), byte << np.uint32(24), np.uint32(0x3f800000) | byte,
                 r.choice(np.array([0, 0x80000000], np.uint32), n), (byte & np.uint32(0x80)) << np.uint32(24) | r.integers(1, 1000, n).astype(np.uint32),
                 with_inf, with_nan]
    return np.stack([kinds[c % len(kinds)].view(np.uint32) for c in range(d)], axis=1)


def dev(words, is_int, pad=0):
    """The table on the device with row stride d + pad (the padding holds NaN words / INT_MIN)."""
    n, d = words.shape
    buf = np.full((n, d + pad), NEG_NAN if not is_int else 0x80000000, np.uint32)
    buf[:, :d] = words
    t = torch.tensor(buf.view(np.int32), device="cuda")
    return (t if is_int else t.view(torch.float32))[:, :d]


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("is_int,pad", [(False, 0), (False, 3), (True, 0), (True, 3)])
@pytest.mark.parametrize("n,d", _shapes())
def test_sort_and_midranks_equal_the_reference_by_value(gpu, n, d, is_int, pad):
    lib = L.load()
    words = table(n, d, is_int, seed=n * 131 + d)
    x = dev(words, is_int, pad)
    want_sorted, want_ranks = UR.sort_columns(words, is_int), UR.ranks2(words, is_int)
    assert np.array_equal(bits(UV.sort_columns(x)), want_sorted)
    assert np.array_equal(UV.midranks(x).cpu().numpy(), want_ranks)
    # the entry again, on a workspace and outputs pre-filled with 0xFF
    ws = torch.full((lib.d3p_sort_columns_workspace(n, d, 1),), 0xff, dtype=torch.uint8, device="cuda")
    out, ranks = torch.full((d, n + 5), -1, dtype=torch.int32, device="cuda"), torch.full((n, d + 2), -1, dtype=torch.int32, device="cuda")
    L.check(lib.d3p_sort_columns(L.stream_ptr(), L.ptr(x), int(is_int), d + pad, n, d, L.ptr(out), n + 5, L.ptr(ranks), d + 2, L.ptr(ws), ws.numel()))
    assert np.array_equal(bits(out[:, :n]), want_sorted) and bool((out[:, n:] == -1).all())
    assert np.array_equal(ranks[:, :d].cpu().numpy(), want_ranks) and bool((ranks[:, d:] == -1).all())
    if not is_int and d >= 11:
        assert not want_ranks[:, 10].any() and want_ranks[:, 9].all() and want_ranks[:, 0].all()   # the NaN column is 0, its neighbours are not
    unsorted_keys = ws[:4 * n * d].view(torch.int32).view(d, n).cpu().numpy().view(np.uint32)      # W0 still holds the unsorted keys
    assert np.array_equal(unsorted_keys, UR.keys(words, is_int).T)


def test_spearman_is_the_correlation_of_the_midranks(gpu):
    x = dev(table(4097, 13, False, seed=5), False, 3)
    assert np.array_equal(UV.spearman(x).cpu().numpy(), CV.correlation(UV.midranks(x)).cpu().numpy(), equal_nan=True)
    r = np.random.default_rng(3)
    cols = np.stack([r.permutation(65) for _ in range(3)], axis=1).astype(np.float32)          # no ties: the textbook formula
    got = UV.spearman(torch.tensor(cols, device="cuda")).cpu().numpy()
    for c in range(3):
        for e in range(3):
            delta = (cols[:, c] - cols[:, e]).astype(np.float64)
            assert abs(got[c, e] - (1.0 - 6.0 * float(delta @ delta) / (65 * (65 ** 2 - 1)))) <= 1e-12


def cdf_tables(na, nb, is_int, seed):
    """Two (n, 5 or 7) word tables: identical (n_a == n_b) or resampled, disjoint, interleaved, heavily tied, normal; float32: +-inf, NaN."""
    r = np.random.default_rng(seed)
    cast = (lambda v: np.asarray(v).astype(np.int32).view(np.uint32)) if is_int else (lambda v: np.asarray(v).astype(np.float32).view(np.uint32))
    base = r.normal(size=max(na, nb)) * 1000.0
    a = [base[:na], r.normal(size=na) * 50.0 - 1000.0, 2.0 * np.arange(na), r.integers(0, 4, na), r.normal(size=na) * 1000.0]
    b = [np.resize(base[:na], nb), r.normal(size=nb) * 50.0 + 1000.0, 2.0 * np.arange(nb) + 1.0, r.integers(1, 6, nb), r.normal(size=nb) * 1000.0 + 300.0]
    a, b = [cast(v) for v in a], [cast(v) for v in b]
    if not is_int:
        for extra in ((NEG_INF, POS_INF), (POS_NAN, NEG_NAN)):
            ca, cb = a[4].copy(), b[4].copy()
            ca[r.integers(0, na)], cb[r.integers(0, nb)] = extra
            a.append(ca), b.append(cb)
    return np.stack(a, axis=1), np.stack(b, axis=1)


worst_ratio = 0.0


@pytest.mark.parametrize("is_int", [False, True])
@pytest.mark.parametrize("na,nb", [(1, 1), (64, 65), (4097, 4096), (20001, 8193), (4097, 4097)])
def test_cdf_distance_against_the_integer_and_fsum_reference(gpu, na, nb, is_int):
    global worst_ratio
    lib = L.load()
    wa, wb = cdf_tables(na, nb, is_int, seed=na + nb)
    got = UV.cdf_distance(dev(wa, is_int, 3), dev(wb, is_int))
    num, at, w1 = got.ks_num.cpu().numpy(), bits(got.ks_at), got.w1.cpu().numpy()
    for c in range(5):
        want_num, want_key, want_w1, sum_abs = UR.cdf_column(wa[:, c], wb[:, c], is_int)
        bound = UR.w1_bound(lib, na, nb, sum_abs)
        ratio = abs(w1[c] - want_w1) / bound if bound else 0.0
        worst_ratio = max(worst_ratio, ratio)
        print(f"cdf n_a={na} n_b={nb} int={is_int} col={c}: ks_num={num[c]} w1={w1[c]!r} ref={want_w1!r} error/bound={ratio:.3g} (worst {worst_ratio:.3g})")
        assert num[c] == want_num and UR.keys(at[c:c + 1], is_int)[0] == want_key
        assert abs(w1[c] - want_w1) <= bound
    assert num[1] == na * nb and float(got.ks[1]) == 1.0                                         # disjoint: ks = 1 exactly
    if na == nb:
        assert num[0] == 0 and w1[0] == 0.0 and float(got.ks[0]) == 0.0                          # identical tables
    if not is_int:
        want_num = UR.cdf_column(wa[:, 5], wb[:, 5], is_int)[0]
        assert num[5] == want_num and math.isnan(w1[5]) and float(got.ks[5]) == want_num / (na * nb)   # +-inf: a valid KS, w1 NaN
        assert num[6] == -1 and math.isnan(w1[6]) and math.isnan(float(got.ks[6])) and UR.is_nan(at[6:7])[0]


def test_univariate_fidelity_names_the_shifted_column_and_the_broken_pair(gpu):
    r = np.random.default_rng(11)

    def draw(n):
        z = r.normal(size=(n, 4))
        z[:, 1] = np.exp(z[:, 0]) + 0.05 * z[:, 1]                                             # columns 0 and 1: monotone dependence
        return z
    real, synth, hold = draw(3001), draw(2500), draw(1500)
    synth[:, 2] += 1.5                                                                         # column 2 shifted
    synth[:, 1] = r.permutation(synth[:, 1])                                                   # the pair (0, 1) broken, the marginal kept
    t = [torch.tensor(v.astype(np.float32), device="cuda") for v in (real, synth, hold)]
    rep = UV.univariate_fidelity(t[0], t[1], holdout=t[2], top=2)
    assert rep.worst_columns[0][0] == 2 and rep.worst_pairs[0][0] == (0, 1) and rep.n_pairs_skipped == 0 and rep.floor.floor is None
    assert float(rep.floor.ks.max()) < rep.worst_columns[0][1] and rep.floor.spearman_diff_max < rep.spearman_diff_max
    assert float(rep.w1_scaled[2]) > float(rep.floor.w1_scaled[2]) and (rep.n_real, rep.n_synthetic, rep.dim) == (3001, 2500, 4)
