"""d3p_amd.sliced on the GPU against tests/sliced_ref.py: bounds derived in d3p_sliced.hip's header, determinism by bits, end to end."""
import numpy as np
import pytest
import torch

import d3p_amd._lib as L
from d3p_amd import covariance as CV
from d3p_amd import sliced as SL
from d3p_amd import univariate as UV
from tests import sliced_ref as SR

pytestmark = pytest.mark.gpu
NAN_WORD, INT_MIN, SENTINEL = 0xffc00001, 0x80000000, -7.5


LIB = L.load()      # the geometry comes from the query functions (host-only: callable while collecting)
R, K, D, T = LIB.d3p_project_rows_tile_rows(), LIB.d3p_project_rows_chunk_cols(), LIB.d3p_project_rows_max_launch_dirs(), LIB.d3p_sort_columns_block_keys()
PROJECTION_SHAPES = ([(n, K + 1, 33) for n in (1, 31, 32, 33, R - 1, R, R + 1, 2 * R + 5)] + [(R + 1, d, 33) for d in (1, 2, 3, K - 1, K, K + 1, 2 * K + 3)]
                     + [(33, K + 1, dirs) for dirs in (1, 31, 32, 33, D, D + 1)])
W2_SHAPES = [(1, 1), (1, 5), (5, 1), (7, 7), (T - 1, T + 1), (T + 1, 3), (4 * 1031, 1031), (2 * T + 17, T - 3)]


def table(n, d, is_int, seed):
    """(n, d) values: normal data, and column 0 at offset 10^6 with unit spread."""
    r = np.random.default_rng(seed)
    x = r.normal(size=(n, d)) * (100.0 if is_int else 1.0)
    x[:, 0] = 1e6 + r.normal(size=n) * (3.0 if is_int else 1.0)
    return np.rint(x).astype(np.int32) if is_int else x.astype(np.float32)


def dev(values, pad=0):
    """The (rows, cols) array on the device with row stride cols + pad; the padding holds NaN words (INT_MIN for int32)."""
    n, d = values.shape
    buf = np.full((n, d + pad), INT_MIN if values.dtype == np.int32 else NAN_WORD, np.uint32)
    buf[:, :d] = values.view(np.uint32)
    t = torch.tensor(buf.view(np.int32), device="cuda")
    return (t if values.dtype == np.int32 else t.view(torch.float32))[:, :d]


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32).cpu().numpy()


@pytest.mark.parametrize("is_int,shifted,pad", [(i, s, p) for i in (False, True) for s in (False, True) for p in (0, 3)])
@pytest.mark.parametrize("n,d,dirs", PROJECTION_SHAPES)
def test_projection_is_within_the_headers_bound(gpu, n, d, dirs, is_int, shifted, pad):
    x = table(n, d, is_int, seed=n * 131 + d * 7 + dirs)
    theta = SL.random_directions(d, dirs, seed=d).numpy()
    shift = x.astype(np.float64).mean(axis=0).astype(np.float32) if shifted else None
    want, bound = SR.project(x, theta, shift, K)
    xd, td = dev(x, pad), dev(theta, pad)
    sd = torch.tensor(shift, device="cuda") if shifted else None
    out = torch.full((n, dirs + pad), SENTINEL, dtype=torch.float32, device="cuda")
    L.check(LIB.d3p_project_rows(L.stream_ptr(), L.ptr(xd), int(is_int), d + pad, n, d, L.ptr(td), dirs + pad, dirs, L.ptr(sd), L.ptr(out), dirs + pad))
    got = out.cpu().numpy().astype(np.float64)
    ratio = float((np.abs(got[:, :dirs] - want) / bound).max())
    print(f"largest error / bound = {ratio:.3f} (n, d, L = {n}, {d}, {dirs}; int32 {is_int}, shift {shifted}, pad {pad})")
    assert ratio <= 1.0
    assert (got[:, dirs:] == SENTINEL).all()                       # nothing beyond p[i][0 .. L) is written
    if not pad:
        assert np.array_equal(bits(SL.project(xd, td, sd)), bits(out))


def test_projection_bits_do_not_depend_on_the_launch(gpu):
    n, d, dirs = 2 * R + 5, K + 1, D + 33
    x, theta = table(n, d, False, seed=5), SL.random_directions(d, dirs, seed=9)
    x[R, 5] = np.nan
    shift = torch.tensor(x[:, :].astype(np.float64).mean(axis=0).astype(np.float32)).nan_to_num(0.0).cuda()
    xd = dev(x, 3)                                                  # ld = K + 4: the 16-byte loads
    big = SL.project(xd, theta.cuda(), shift)
    assert bool(big[R].isnan().all()) and not bool(big[R - 1].isnan().any()) and not bool(big[R + 1].isnan().any())
    rows, cols = slice(R - 1, R + 40), slice(D - 1, D + 20)         # other strips, tiles, slab positions, L, ld (one word a lane), ld_t
    small = SL.project(dev(x[rows]), theta[:, cols].contiguous().cuda(), shift)
    assert np.array_equal(bits(small), bits(big[rows, cols]))


def sorted_table(n, d, is_int, seed):
    """(d, n) sorted columns: normal data, odd columns rounded so that they hold ties."""
    r = np.random.default_rng(seed)
    x = r.normal(size=(d, n)) * (50.0 if is_int else 1.0)
    x[1::2] = np.rint(x[1::2] * 4.0) / 4.0
    return np.sort(np.rint(x).astype(np.int32) if is_int else x.astype(np.float32), axis=1)


@pytest.mark.parametrize("is_int", [False, True])
@pytest.mark.parametrize("d", [1, 65])
@pytest.mark.parametrize("n_a,n_b", W2_SHAPES)
def test_w2_distance_is_within_its_roundings_of_the_walk(gpu, n_a, n_b, d, is_int):
    a, b = sorted_table(n_a, d, is_int, seed=n_a * 3 + d), sorted_table(n_b, d, is_int, seed=n_b * 5 + d + 1)
    ad, bd = dev(a, 2), dev(b)
    got = SL.w2_distance(ad, bd)
    worst = 0.0
    for c in range(d):
        want, sum_abs = SR.wasserstein(a[c], b[c], 2)
        err, bound = abs(float(got[c]) - want), SR.w2_bound(LIB, n_a, n_b, sum_abs)
        worst = max(worst, err / bound if bound else (np.inf if err else 0.0))       # (equal values: a bound of 0, met exactly)
    print(f"largest error / bound = {worst:.3f} (n_a, n_b, d = {n_a}, {n_b}, {d}; int32 {is_int})")
    assert worst <= 1.0
    assert np.array_equal(bits(SL.w2_distance(bd, ad)), bits(got))            # swapped
    assert not bool(SL.w2_distance(ad, dev(a)).any())                         # equal tables: exactly 0
    for short, want in ((0, got), (1, torch.full_like(got, SENTINEL))):        # stale workspace bytes change nothing; a byte short: refused, untouched
        ws = torch.full((LIB.d3p_column_w2_distance_workspace(n_a, n_b, d),), 0xff, dtype=torch.uint8, device="cuda")
        out = torch.full_like(got, SENTINEL)
        rc = LIB.d3p_column_w2_distance(L.stream_ptr(), L.ptr(ad), n_a + 2, n_a, L.ptr(bd), n_b, n_b, int(is_int), d, L.ptr(out), L.ptr(ws), ws.numel() - short)
        assert rc == (-4 if short else 0) and np.array_equal(bits(out), bits(want))


@pytest.mark.parametrize("in_b,last,word", [(False, False, 0xff800000), (False, True, 0x7f800000), (True, False, NAN_WORD), (True, True, 0x7fc00000)])
def test_w2_distance_flags_a_non_finite_column_alone(gpu, in_b, last, word):
    a, b = sorted_table(T + 1, 3, False, seed=1), sorted_table(77, 3, False, seed=2)
    clean = SL.w2_distance(dev(a), dev(b))
    (b if in_b else a).view(np.uint32)[1, -1 if last else 0] = word
    got = SL.w2_distance(dev(a), dev(b))
    assert bool(got[1].isnan()) and np.array_equal(bits(got[[0, 2]]), bits(clean[[0, 2]])) and not bool(clean.isnan().any())


def test_sliced_wasserstein_end_to_end(gpu):
    n_a, n_b, d, dirs = T + 1, 1000, 5, 33
    real, synth = table(n_a, d, False, seed=11), table(n_b, d, False, seed=12) * np.float32(1.25)
    rd, sd = dev(real), dev(synth, 3)
    got = SL.sliced_wasserstein(rd, sd, n_dirs=dirs, scale=None)
    theta = SL.random_directions(d, dirs, seed=0).numpy()
    shift = CV.column_moments(rd).mean.to(torch.float32).cpu().numpy()
    (pa, ea), (pb, eb) = SR.project(real, theta, shift, K), SR.project(synth, theta, shift, K)
    w1, w2, tol1, tol2 = (np.zeros(dirs) for _ in range(4))
    k1, k2 = LIB.d3p_column_cdf_distance_roundings(n_a, n_b) + 4, LIB.d3p_column_w2_distance_roundings(n_a, n_b) + 6
    for l in range(dirs):
        a, b = np.sort(pa[:, l]), np.sort(pb[:, l])
        w1[l], w2[l] = SR.wasserstein(a, b, 1)[0], SR.wasserstein(a, b, 2)[0] ** 0.5
        # W_p moves by at most the largest move of a point, on either side; then the float64 roundings of sums of terms >= 0, both sides'
        moved = ea[:, l].max() + eb[:, l].max()
        tol1[l], tol2[l] = moved + 2 * k1 * SR.U64 * (w1[l] + moved), moved + (k2 + 2) * SR.U64 * (w2[l] + moved)
    got_w2 = got.w2sq.sqrt().cpu().numpy()
    assert (np.abs(got.w1.cpu().numpy() - w1) <= tol1).all() and (np.abs(got_w2 - w2) <= tol2).all()
    # the mean of w1; the root mean square of w2 (Minkowski: at most the largest per-direction move), a few float64 roundings each
    assert abs(got.sw1 - w1.mean()) <= tol1.mean() + 2 * dirs * SR.U64 * w1.mean()
    assert abs(got.sw2 - np.sqrt(np.mean(w2 ** 2))) <= tol2.max() + 2 * dirs * SR.U64 * w2.max()
    assert (got.max_w1, got.max_w1_at, got.max_w2) == (float(got.w1.max()), int(got.w1.argmax()), float(got.w2sq.max().sqrt()))
    slabs = SL.sliced_wasserstein(rd, sd, n_dirs=dirs, scale=None, slab_bytes=4 * (n_a + n_b) * 11)    # three slabs of 11
    for name in ("w1", "w2sq", "ks"):
        assert np.array_equal(bits(getattr(slabs, name)), bits(getattr(got, name))), name
    same = SL.sliced_wasserstein(rd, dev(real, 1), n_dirs=dirs, holdout=sd)
    assert same.sw1 == same.sw2 == 0.0 and same.floor.n_synthetic == n_b and same.floor.sw2 > 0.0
    # one column, the direction 1.0, no shift: the projection is the (normal) data itself
    one = torch.ones((1, 1), device="cuda")
    assert np.array_equal(bits(UV.cdf_distance(SL.project(rd[:, 1], one), SL.project(sd[:, 1], one)).w1), bits(UV.cdf_distance(rd[:, 1], sd[:, 1]).w1))
