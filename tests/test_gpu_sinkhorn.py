"""d3p_amd.sinkhorn on the GPU against tests/sinkhorn_ref.py within the bound d3p_sinkhorn.hip's header derives; the running reference,
flags, bits, workspace, end to end."""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

import d3p_amd._lib as L
from d3p_amd import sinkhorn as S
from tests import sinkhorn_ref as SR
from tests import workspace_harness as H
from tests.test_gpu_mmd import NAN_WORD, dev, table

pytestmark = pytest.mark.gpu
LIB = L.load()      # the geometry comes from the query functions (host-only: callable while collecting)
T, GROUP, RES = 32, LIB.d3p_softmin_rows_group_tiles() * 32, LIB.d3p_softmin_rows_resident_cols()
INF = np.float32(np.inf)
# (na, nb, d, int32, stride, coefficients, forced segments, prev with omega 1/2, logw); stride as tests/test_gpu_mmd.py's dev
_N, _D = (1, 31, 32, 33, 127, 128, 129), (1, 2, 3, 31, 32, 33, 65, RES - 1, RES, RES + 1)
CASES = [(_N[k % 7], _N[(3 * k + 2) % 7], d, k % 2 == 1, k % 3, k % 4 < 2, (0, 1, 2)[k % 3], k % 2 == 0, k % 3 != 1) for k, d in enumerate(_D)]
CASES += [(33, nb, d, False, 1, True, 1, True, True) for nb, d in ((GROUP - 1, 3), (GROUP, RES), (GROUP + 1, RES + 1))]       # the float32 group's edge
CASES += [(129, 129, 33, False, 0, True, 2, False, True), (127, 2 * T * 3 + 1, 2, True, 1, True, 2, True, False)]             # a segment's edge


def inputs(na, nb, d, is_int, given, with_prev, with_logw):
    """(a, b, shift, scale, gamma, h, prev, logw) in numpy: epsilon 5 % of the typical squared distance 2 d, h a few bits wide."""
    a, b = table(na, d, is_int, seed=na * 131 + d, offset=1e4 if given else 0.0), table(nb, d, is_int, seed=nb * 7 + d + 1, offset=1e4 if given else 0.0)
    shift, scale = (b.astype(np.float64).mean(axis=0).astype(np.float32), np.linspace(0.5, 1.5, d).astype(np.float32)) if given else (None, None)
    r = np.random.default_rng(na + 3 * nb + d)
    gamma = 1.0 / (2.0 * np.log(2.0) * 0.05 * 2.0 * d * (9.0 if is_int else 1.0))
    return (a, b, shift, scale, gamma, (3.0 * r.normal(size=nb)).astype(np.float32), 5.0 * r.normal(size=na) if with_prev else None,
            (-np.log2(na) + r.normal(size=na)).astype(np.float32) if with_logw else None)


def cuda(v):
    return None if v is None else torch.tensor(v, device="cuda")


def forced(segments, fn):
    assert LIB.d3p_softmin_rows_set_segments(segments) == 0
    try:
        return fn()
    finally:
        LIB.d3p_softmin_rows_set_segments(0)


def guarded(fill, fn, short_by=0):
    """fn() with softmin_rows' outputs and workspace taken from guarded, pre-filled memory."""
    rec, mp = H.Recorder(fill, short_by, None), pytest.MonkeyPatch()
    H.guarded_empty(mp, S, rec, "softmin_rows")
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        mp.undo()
    rec.check_all()
    return out


def within(got, a, b, gamma, h, shift=None, scale=None, prev=None, omega=1.0, segments=0):
    """Asserts pot within the bound of the reference; returns the largest error / bound."""
    rounds = forced(segments, lambda: LIB.d3p_softmin_rows_roundings(len(a), len(b)))
    want, bound = SR.softmin_rows(a, b, gamma, h, shift, scale, prev, omega, None, rounds)
    err = np.abs(got.cpu().numpy() - want)
    assert bool((err <= bound).all()), float((err / bound).max())
    return float((err / bound).max())


@pytest.mark.parametrize("na,nb,d,is_int,stride,given,segments,with_prev,with_logw", CASES)
def test_softmin_rows_are_within_the_headers_bound(gpu, na, nb, d, is_int, stride, given, segments, with_prev, with_logw):
    a, b, shift, scale, gamma, h, prev, logw = inputs(na, nb, d, is_int, given, with_prev, with_logw)
    ad, bd, rest = dev(a, stride), dev(b, (stride + 1) % 3), (cuda(h), cuda(shift), cuda(scale), cuda(prev), 0.5 if with_prev else 1.0, cuda(logw))

    def run(fill="bits", short_by=0, x=ad, y=bd):
        return forced(segments, lambda: guarded(fill, lambda: S.softmin_rows(x, y, gamma, *rest), short_by))
    pot, out_h = run()
    print(f"largest error / bound = {within(pot, a, b, gamma, h, shift, scale, prev, 0.5, segments):.3f}")
    assert pot.shape == (na,) and (out_h is None) == (logw is None)
    if with_logw:                                                  # out_h is the float32 of pot + logw, to the bit
        assert np.array_equal(out_h.cpu().numpy(), SR.out_h(pot.cpu().numpy(), logw))
    again = run("ones")                                            # stale workspace bytes change nothing; repeated calls give equal bits
    assert torch.equal(H.raw_bytes(again[0]), H.raw_bytes(pot))
    with pytest.raises(L.D3PError, match="workspace too small"):   # a byte short: refused
        run("zero", short_by=1)
    if stride:                                                     # the bits of a row do not depend on the strides or the load form
        assert torch.equal(H.raw_bytes(run(x=dev(a), y=dev(b))[0]), H.raw_bytes(pot))


@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_the_running_reference_under_every_order_of_h(gpu, order):
    """h climbs 40 bits a tile: ascending, every tile raises every lane's reference; descending, none after the first."""
    a, b = table(40, 3, False, 11, 0.0), table(6 * T + 5, 3, False, 12, 0.0)
    h = (40.0 * (np.arange(len(b)) // T)).astype(np.float32)
    h = {"ascending": h, "descending": h[::-1].copy(), "permuted": np.random.default_rng(5).permutation(h)}[order]
    got = forced(1, lambda: S.softmin_rows(dev(a), dev(b, 1), 0.3, cuda(h)))[0]
    print(f"largest error / bound = {within(got, a, b, 0.3, h, segments=1):.3f}")


@pytest.mark.parametrize("d", [3, RES + 1])
def test_a_wave_divergent_rescale_changes_no_bit(gpu, d):
    """b's last tile holds one row next to a[7] and far from every other row of a: at that tile row 7's references rise and no other's,
    so the other rows are rescaled by 2^0.  Both kinds of row keep the bits of the row walked alone."""
    a, b = table(40, d, False, 13, 0.0), table(3 * T, d, False, 14, 0.0)
    a[7] += np.float32(6.0)
    b[2 * T + 9] = a[7]
    h, bd = cuda(np.zeros(len(b), np.float32)), dev(b)
    got = S.softmin_rows(dev(a), bd, 1.0, h)[0]
    within(got, a, b, 1.0, np.zeros(len(b), np.float32))
    for i in (7, 0):
        assert torch.equal(H.raw_bytes(S.softmin_rows(dev(a[i:i + 1]), bd, 1.0, h)[0]), H.raw_bytes(got[i:i + 1]))


@pytest.mark.parametrize("d", [3, RES + 1])
def test_zero_weights_duplicates_far_rows_and_non_finite_values(gpu, d):
    a, b = table(70, d, False, 3, 0.0), table(2 * T + 5, d, False, 4, 0.0)
    b[7], b[40] = a[2], a[2]                                       # duplicates: q clamped, never negative
    a[5] = np.sqrt(400.0 / d)                                      # a far row of a: every term lies some 200 bits below its h
    b[50] = -np.sqrt(1200.0 / d)                                   # a far row of b: its term lies 500 bits below the others and underflows
    h = np.random.default_rng(9).normal(size=len(b)).astype(np.float32)
    h[3], h[-2:] = -INF, -INF                                      # zero weights: ignored; at the tail of the last tile as if not there
    ad, bd = dev(a, 1), dev(b)
    got = S.softmin_rows(ad, bd, 0.5, cuda(h))[0]
    within(got, a, b, 0.5, h)
    assert torch.equal(H.raw_bytes(S.softmin_rows(ad, dev(b[:-2]), 0.5, cuda(h[:-2]))[0]), H.raw_bytes(got))
    assert float(got[5]) > 100.0 > float(got[:5].max())
    none = S.softmin_rows(ad, bd, 0.5, cuda(np.full(len(b), -INF)))[0]
    assert bool((none == float("inf")).all())                      # every weight zero: pot = +inf, no NaN
    for word in (np.float32(np.nan), INF):
        bad = h.copy()
        bad[1] = word
        assert bool(S.softmin_rows(ad, bd, 0.5, cuda(bad))[0].isnan().all())
    clean = H.raw_bytes(got[:4])
    for word, in_b in ((NAN_WORD, False), (0x7f800000, False), (0xff800000, True), (0x7fc00000, True)):
        x = (b if in_b else a).copy()
        x.view(np.uint32)[4, d - 1] = word
        bad = S.softmin_rows(dev(x if not in_b else a), dev(x if in_b else b, 2), 0.5, cuda(h))[0]
        if in_b:
            assert bool(bad.isnan().all())
        else:
            assert bool(bad[4].isnan()) and not bool(bad[:4].isnan().any()) and not bool(bad[5:].isnan().any())
            assert torch.equal(H.raw_bytes(bad[:4]), clean)


def test_sinkhorn_divergence_end_to_end(gpu):
    """Against the dense float64 iteration with the same schedule.  Soft-min is non-expansive in the sup norm and an averaged step a convex
    combination, so a potential errs by at most (walks on the path) x (the largest per-walk bound, with the rounding of the float32 h it
    read, in cost units); a value, a weighted sum of two potentials (four with debias), by twice (four times) that."""
    x, y = table(150, 4, False, 5), (table(90, 4, False, 6) * np.float32(1.0002)).astype(np.float32)
    r = np.random.default_rng(7)
    wx, wy = r.uniform(0.5, 1.5, 150), r.uniform(0.5, 1.5, 90)
    wx[17] = 0.0
    xd, yd = dev(x, 1), dev(y, 2)
    got = S.sinkhorn_divergence(xd, yd, epsilon=0.4, wx=cuda(wx), wy=cuda(wy), n_iter=6, check_every=100)
    mom = S.CV.column_moments(xd)
    shift, scale = mom.mean.float().cpu().numpy(), (1.0 / (mom.m2.diagonal() / 149.0).sqrt()).float().cpu().numpy()
    rungs = SR.schedule(x, y, shift, scale, 0.4, 0.5)
    div, ot, f, g, worst, walks = SR.sinkhorn(x, y, 0.4, wx, wy, shift, scale, rungs, 6)
    tol = walks * worst
    print(f"{len(rungs)} rungs, tolerance of a potential {tol:.3e}, divergence {div:.6f}")
    assert len(rungs) >= 2 and got.n_iter_run == 6 and not got.converged and got.epsilon == 0.4 and got.marginal_error >= 0.0
    assert np.abs(got.f_x.cpu().numpy() - f).max() <= tol and np.abs(got.g_y.cpu().numpy() - g).max() <= tol
    assert abs(float(got.ot_xy) - ot) <= 2 * tol and abs(float(got.divergence) - div) <= 4 * tol
    plain = S.sinkhorn_divergence(xd, yd, epsilon=0.4, wx=cuda(wx), wy=cuda(wy), n_iter=6, check_every=100, debias=False)
    assert float(plain.divergence) == float(plain.ot_xy) and abs(float(plain.ot_xy) - ot) <= 2 * tol
    same = S.sinkhorn_divergence(xd, dev(x), epsilon=0.4, n_iter=6, check_every=100)
    assert abs(float(same.divergence)) <= 4 * tol                  # equal tables: within the tolerance of 0
    one = S.sinkhorn_divergence(dev(x[:1]), dev(y[:1]), epsilon=0.4, n_iter=6, check_every=100, scale=None)
    cost = 0.5 * float(((y[:1].astype(np.float64) - x[:1]) ** 2).sum())
    assert abs(float(one.divergence) - cost) <= 4 * tol and abs(float(one.ot_xy) - cost) <= 2 * tol


def test_the_example_prints_its_line(gpu, capsys):
    spec = importlib.util.spec_from_file_location("ex_gmm_sinkhorn", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples",
                                                                                 "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["--sinkhorn"]).sinkhorn == 0.05 and mod.parse_args(["--sinkhorn", "0.1"]).sinkhorn == 0.1 and mod.parse_args([]).sinkhorn is None
    mod.main(argparse.Namespace(num_epochs=2, learning_rate=5e-2, batch_size=64, dimensions=2, num_samples=512, num_components=3, sigma=0.3, sinkhorn=0.1))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Sinkhorn divergence (epsilon")]
    assert len(lines) == 1 and "512 synthetic rows): " in lines[0] and "ot_xy" in lines[0] and "converged" in lines[0] and "held-out floor" in lines[0]
