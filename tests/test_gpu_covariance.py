"""d3p_column_moments and d3p_amd.covariance on the GPU against tests/covariance_ref.py (exact cases, the derived bound, bit equality)."""
import argparse
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import d3p_amd._lib as L
from tests import covariance_ref as CR
from tests import workspace_harness as WH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def LIB(gpu):
    return L.load()


def _shapes():   # the issue's edge shapes, crossed sparsely, from the query functions (host-only: callable while collecting)
    lib = L.load()
    B, Ls, R, _ = CR.geometry(lib, 1, 1)          # (R: the shortest segment, which every n of this list has)
    ns = (1, 2, 3, 7, 8, 9, 4 * Ls - 1, 4 * Ls, 4 * Ls + 1, R - 1, R, R + 1, 2 * R + 1)
    ds = (1, 2, 31, 32, 33, B - 1, B, B + 1, 2 * B + 1)
    cases = [(n, ds[i % len(ds)]) for i, n in enumerate(ns)] + [(2 * R + 1, 2 * B + 1), (R + 1, B + 1), (4 * Ls + 1, 33), (9, 784)]
    assert all(CR.geometry(lib, n, d)[2] == R for n, d in cases)
    return list(dict.fromkeys(cases))


def entry(LIB, x, pad=0, m2_pad=0, fill="ones", short_by=0, expect=0):
    """d3p_column_moments on x with ld = d + pad, m2_ld = d + m2_pad, outputs and workspace pre-filled between guards: (mean, m2)."""
    n, d = x.shape
    xb = torch.full((n, d + pad), 77, dtype=torch.int32 if x.dtype == np.int32 else torch.float32, device="cuda")
    xb[:, :d] = torch.tensor(x)
    before = xb.clone()
    rec = WH.Recorder(fill, short_by, None)
    mean, m2 = rec.take(8 * d, "cuda", "mean", output=True), rec.take(8 * d * (d + m2_pad), "cuda", "m2", output=True)
    ws = rec.take(int(LIB.d3p_column_moments_workspace(n, d)), "cuda", "ws")
    rc = LIB.d3p_column_moments(L.stream_ptr(), L.ptr(xb), int(x.dtype == np.int32), d + pad, n, d, L.ptr(mean.interior), L.ptr(m2.interior),
                                d + m2_pad, L.ptr(ws.interior), ws.nbytes)
    torch.cuda.synchronize()
    assert rc == expect, (rc, LIB.d3p_last_error())
    rec.check_all("d3p_column_moments")
    assert torch.equal(WH.raw_bytes(xb), WH.raw_bytes(before)), "the table was written"
    if expect != 0:
        for g in rec.buffers:
            assert torch.equal(g.interior.cpu(), WH._fill_bytes(g.nbytes, g.fill, seed=g.seed)), g.tag
        return None
    full = m2.interior.view(torch.float64).view(d, d + m2_pad).cpu()
    assert bool(torch.isnan(full[:, d:]).all()), "the padding of m2 was written"       # (0xFF bytes are NaN)
    return mean.interior.view(torch.float64).cpu().numpy().copy(), full[:, :d].numpy().copy()


def float_table(n, d, seed):
    """Means up to 10^6 times the spread; column 0 constant (d >= 2); columns 2 and 3 with correlation -1 (d >= 4)."""
    rng = np.random.default_rng(seed)
    spread = 10.0 ** rng.uniform(-2, 2, d)
    x = (spread * 10.0 ** np.linspace(0, 6, d) * rng.choice([-1.0, 1.0], d) + spread * rng.normal(size=(n, d))).astype(np.float32)
    if d >= 2:
        x[:, 0] = np.float32(3.25e5)
    if d >= 4:
        x[:, 3] = -x[:, 2]
    return x


@pytest.mark.parametrize("dtype", [np.float32, np.int32], ids=["float32", "int32"])
@pytest.mark.parametrize("n,d", _shapes())
def test_integer_tables_bit_for_bit(LIB, n, d, dtype):
    x, mean, m2 = CR.exact_table(n, d, dtype, seed=n * 1000 + d)
    got = entry(LIB, x, pad=3, m2_pad=5)
    assert np.array_equal(got[0], mean), "a mean is not its integer (s is not exactly 0, or a row or column was dropped or doubled)"
    assert np.array_equal(got[1], m2), np.argwhere(got[1] != m2)[:5].tolist()


@pytest.mark.parametrize("n,d", _shapes())
def test_general_floats_inside_the_derived_bound(LIB, n, d):
    x = float_table(n, d, seed=n * 1000 + d)
    _, L, R, nseg = CR.geometry(LIB, n, d)
    (mean, m2), (rmean, rm2), (tmean, tm2) = entry(LIB, x), CR.reference(x), CR.bound(x, L, R, nseg)
    emean, em2 = np.abs(mean - rmean), np.abs(m2 - rm2)
    print(f"n={n} d={d}: largest error / bound: mean {float((emean / tmean).max()):.3g}, m2 {float((em2 / tm2).max()):.3g}")
    assert (emean <= tmean).all() and (em2 <= tm2).all()
    assert d < 2 or not m2[0].any()                                   # the constant column: exactly 0, not a small number
    assert d < 4 or m2[2, 3] == -m2[2, 2] == -m2[3, 3]                # correlation -1 exactly


def test_bits_non_finite_values_and_the_short_workspace(LIB):
    n, d = max(_shapes())      # 2 R + 1 rows of 2 B + 1 columns
    x = float_table(n, d, seed=5)
    mean, m2 = entry(LIB, x)
    assert m2.tobytes() == m2.T.copy().tobytes()
    for kw in (dict(pad=7, m2_pad=3), dict(fill="zero"), dict(fill="bits"), dict(fill="big"), dict()):
        again = entry(LIB, x, **kw)
        assert again[0].tobytes() == mean.tobytes() and again[1].tobytes() == m2.tobytes(), kw
    keep = np.array([0, 5, 33, d // 2, d - 29, d - 1])
    other = float_table(n, d, seed=6) * np.float32(3.0)
    other[:, keep] = x[:, keep]
    omean, om2 = entry(LIB, other)
    assert omean[keep].tobytes() == mean[keep].tobytes() and om2[np.ix_(keep, keep)].tobytes() == m2[np.ix_(keep, keep)].tobytes()
    assert not np.array_equal(om2, m2)
    col, rest = d // 2 + 6, np.arange(d) != d // 2 + 6
    for value in (np.nan, np.inf, -np.inf):                    # in a row of the last strip: that column alone, every other bit as it was
        bad = x.copy()
        bad[-1, col] = value
        bmean, bm2 = entry(LIB, bad)
        assert np.isnan(bmean[col]) and np.isnan(bm2[col]).all() and np.isnan(bm2[:, col]).all(), value
        assert bmean[rest].tobytes() == mean[rest].tobytes() and bm2[np.ix_(rest, rest)].tobytes() == m2[np.ix_(rest, rest)].tobytes(), value
    for fill in ("ones", "bits"):
        assert entry(LIB, x[:300, :70], fill=fill, short_by=1, expect=-4) is None and b"workspace too small" in LIB.d3p_last_error()


def test_python_layer_on_the_device(LIB):
    from d3p_amd import covariance as CV
    x = float_table(1500, 6, seed=9)
    xt = torch.tensor(x).cuda()
    mom = CV.column_moments(xt)
    m2 = mom.m2.cpu().numpy()
    assert np.array_equal(m2, entry(LIB, x)[1]) and torch.equal(CV.covariance(xt, ddof=0), mom.m2 / 1500.0)     # (torch's own quotient)
    corr, q = CV.correlation(xt).cpu().numpy(), np.diagonal(m2)[1:]
    assert np.isnan(corr[0]).all() and np.isnan(corr[:, 0]).all()                     # the constant column
    assert (np.diagonal(corr)[1:] == 1.0).all() and corr[2, 3] == -1.0
    assert (np.abs(corr[1:, 1:] - m2[1:, 1:] / np.sqrt(np.outer(q, q))) <= 4.0 * CR.E).all()      # a product, a square root, a quotient
    with pytest.raises(ValueError, match="beyond 2\\^24"):
        CV.column_moments(torch.full((4, 2), 2 ** 24 + 1, dtype=torch.int32, device="cuda"))
    # a table against itself: zeros, and frechet 0 up to what the CPU solver leaves of the exact 0 on the reference's own moments plus
    # the first-order rounding of a root of eigenvalues known to d E |C|^2: d E |C| kappa(C), 8 of them
    y = torch.tensor(np.ascontiguousarray(x[:, [1, 2, 4, 5]]))
    same = CV.correlation_fidelity(y.cuda(), y.cuda(), top=3)
    assert not same.smd.any() and bool((same.sd_ratio == 1).all()) and same.corr_diff_max == 0.0 and same.corr_diff_frobenius == 0.0
    ymean, ycov = torch.tensor(CR.reference(y.numpy())[0]), torch.tensor(CR.reference(y.numpy())[1] / 1499.0)
    solver, lam = abs(CV._frechet(ymean, ycov, ymean, ycov)), torch.linalg.eigvalsh(ycov)
    assert abs(same.frechet) <= solver + 8 * 4 * CR.E * float(lam[-1]) * float(lam[-1] / lam[0])
    # sign patterns whose centred columns are exactly orthogonal, in integers: exact moments, diagonal covariances, and the closed form
    # sum (mu_r - mu_s)^2 + sum (sigma_r - sigma_s)^2 to fewer than 64 float64 roundings, each relative to at most the sum of the terms
    signs = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
    a = (np.tile(signs, (1000, 1)) * [1, 2, 3] + [0, 5, -1]).astype(np.float32)
    b = (np.tile(signs, (750, 1)) * [2, 1, 3] + [1, 5, -2]).astype(np.float32)
    rep = CV.correlation_fidelity(torch.tensor(a).cuda(), torch.tensor(b).cuda(), holdout=torch.tensor(a[:2000]).cuda())
    (ma, qa), (mb, qb) = CR.reference(a), CR.reference(b)
    sa, sb = np.sqrt(np.diagonal(qa) / 3999.0), np.sqrt(np.diagonal(qb) / 2999.0)
    closed = ((ma - mb) ** 2).sum() + ((sa - sb) ** 2).sum()
    assert abs(rep.frechet - closed) <= 64 * CR.E * (((ma - mb) ** 2).sum() + (sa ** 2).sum() + (sb ** 2).sum())
    assert rep.corr_diff_max == 0.0 and rep.floor.floor is None and rep.floor.n_synthetic == 2000 and rep.floor.frechet < rep.frechet


def test_example_flag_reports_the_correlation_fidelity(gpu, capsys):
    spec = importlib.util.spec_from_file_location("ex_gmm_correlation", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(argparse.Namespace(num_epochs=2, learning_rate=5e-2, batch_size=64, dimensions=2, num_samples=512, num_components=3, sigma=0.3,
                                correlation_fidelity=True))
    added = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("correlation fidelity")]
    assert len(added) == 1 and re.search(r"\(2 columns, \d+ synthetic rows\): largest standardised mean difference [0-9.]+, correlation difference mean [0-9.]+, "
                     r"max [0-9.]+, Frechet distance -?[0-9.]+; held-out floor \(\d+ rows\)", added[0])
    assert mod.parse_args(["--correlation-fidelity"]).correlation_fidelity is True and mod.parse_args([]).correlation_fidelity is False
