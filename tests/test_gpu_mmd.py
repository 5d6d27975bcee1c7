"""d3p_amd.mmd on the GPU against tests/mmd_ref.py within the bound d3p_mmd.hip's header derives; flags, bits, workspace, end to end."""
import argparse
import importlib.util
import os

import numpy as np
import pytest
import torch

import d3p_amd._lib as L
from d3p_amd import mmd as M
from tests import mmd_ref as MR
from tests import workspace_harness as H

pytestmark = pytest.mark.gpu
LIB = L.load()      # the geometry comes from the query functions (host-only: callable while collecting)
T, GROUP, RES = 32, LIB.d3p_kernel_sums_group_tiles() * 32, LIB.d3p_kernel_sums_resident_cols()
NAN_WORD, INT_MIN = 0xffc00001, 0x80000000
# (na, nb, d, B, int32, stride, coefficients, diagonal, forced segments); stride: 0 dense, 1 padded to 16-byte loads, 2 padded and 4 bytes off
_N, _D = (1, 31, 32, 33, 127, 128, 129), (1, 2, 3, 31, 32, 33, 65, RES - 1, RES, RES + 1)
CASES = [(_N[k % 7], _N[(3 * k + 2) % 7], d, (1, 5, 8)[k % 3], k % 2 == 1, k % 3, k % 4 < 2, False, (0, 1, 2)[k % 3]) for k, d in enumerate(_D)]
CASES += [(n, n, d, B, i, s, True, True, f) for n, d, B, i, s, f in ((1, 3, 5, False, 0, 0), (33, RES, 8, True, 1, 2), (129, RES + 1, 1, False, 2, 0))]
CASES += [(33, nb, d, 5, False, 1, True, False, 1) for nb, d in ((GROUP - 1, 3), (GROUP, RES), (GROUP + 1, RES + 1))]         # the float32 group's edge
CASES += [(129, 129, 33, 5, False, 0, True, False, 2), (127, 2 * T * 3 + 1, 2, 8, True, 1, True, False, 2)]                   # a segment's edge


def table(n, d, is_int, seed, offset=1e4):
    """(n, d) values around `offset` with unit spread: uncentred, so the Gram form needs the shift."""
    x = offset + np.random.default_rng(seed).normal(size=(n, d)) * (3.0 if is_int else 1.0)
    return np.rint(x).astype(np.int32) if is_int else x.astype(np.float32)


def dev(values, stride=0):
    """The array on the device: dense, 16-byte aligned with ld a multiple of 4, or ld odd and 4 bytes off; the padding holds NaN words (INT_MIN)."""
    n, d = values.shape
    ld = d if stride == 0 else (d + 7) // 4 * 4 + (stride == 2)
    buf = np.full(n * ld + 1, INT_MIN if values.dtype == np.int32 else NAN_WORD, np.uint32)
    view = buf[stride == 2:][:n * ld].reshape(n, ld)
    view[:, :d] = values.view(np.uint32)
    t = torch.tensor(buf.view(np.int32), device="cuda")
    t = (t if values.dtype == np.int32 else t.view(torch.float32))[int(stride == 2):][:n * ld].reshape(n, ld)[:, :d]
    return t


def coefficients(x, given):
    if not given:
        return None, None, None, None
    shift, scale = x.astype(np.float64).mean(axis=0).astype(np.float32), np.linspace(0.5, 1.5, x.shape[1]).astype(np.float32)
    return shift, scale, torch.tensor(shift, device="cuda"), torch.tensor(scale, device="cuda")


def forced(segments, fn):
    assert LIB.d3p_kernel_sums_set_segments(segments) == 0
    try:
        return fn()
    finally:
        LIB.d3p_kernel_sums_set_segments(0)


def guarded(fill, fn, short_by=0):
    """fn() with mmd's outputs and workspace taken from guarded, pre-filled memory: (result, recorder)."""
    rec, mp = H.Recorder(fill, short_by, None), pytest.MonkeyPatch()
    H.guarded_empty(mp, M, rec, "kernel_sums")
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        mp.undo()
    rec.check_all()
    return out, rec


@pytest.mark.parametrize("na,nb,d,n_b,is_int,stride,given,excl,segments", CASES)
def test_kernel_sums_are_within_the_headers_bound(gpu, na, nb, d, n_b, is_int, stride, given, excl, segments):
    a, b = table(na, d, is_int, seed=na * 131 + d, offset=1e4 if given else 0.0), table(nb, d, is_int, seed=nb * 7 + d + 1, offset=1e4 if given else 0.0)
    if excl:
        b = a
    shift, scale, sd, cd = coefficients(b, given)
    gamma0 = 1.0 / (2.0 ** (0.5 * (n_b - 1)) * 2.0 * d * (9.0 if is_int else 1.0))        # the middle rung near 1 / E q
    ad, bd = dev(a, stride), dev(b, (stride + 1) % 3)

    def run(fill="bits", short_by=0):
        return forced(segments, lambda: guarded(fill, lambda: M.kernel_sums(ad, bd, gamma0, n_b, sd, cd, excl), short_by))
    (got, rec), rounds = run(), forced(segments, lambda: LIB.d3p_kernel_sums_roundings(na, nb))
    want, bound = MR.kernel_sums(a, b, gamma0, n_b, shift, scale, excl, rounds)
    err = np.abs(got.cpu().numpy() - want)
    print(f"largest error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}, bound / sum <= {float((bound / np.maximum(want, 1e-300)).max()):.2e}")
    assert bool((err <= bound).all()) and got.shape == (n_b, na)              # (no admissible j: 0 within a bound of 0)
    again, _ = run("ones")                                         # stale workspace bytes change nothing; repeated calls give equal bits
    assert torch.equal(H.raw_bytes(again), H.raw_bytes(got))
    with pytest.raises(L.D3PError, match="workspace too small"):   # a byte short: refused
        run("zero", short_by=1)
    if not excl and stride:                                        # the bits of a row do not depend on the strides or the load form
        dense = forced(segments, lambda: M.kernel_sums(dev(a), dev(b), gamma0, n_b, sd, cd))
        assert torch.equal(H.raw_bytes(dense), H.raw_bytes(got))


def test_the_reference_passes_its_own_bound_on_an_uncentred_table_only_with_the_shift():
    """Columns at 10^4 +- 1 (CPU only): the rule in float32 numpy is within the bound of the float64 reference with the shift, and the
    Gram form without it is not."""
    a, b = table(40, 5, False, 1), table(50, 5, False, 2)
    shift = b.astype(np.float64).mean(axis=0).astype(np.float32)
    bound_shifted = MR.kernel_sums(a, b, 0.1, 5, shift)[1]
    for sh, inside in ((shift, True), (None, False)):
        want, bound = MR.kernel_sums(a, b, 0.1, 5, sh)
        err = np.abs(MR.gram_f32(a, b, 0.1, 5, sh) - want)
        assert bool((err <= bound).all()) and bool((err <= bound_shifted).all()) == inside


@pytest.mark.parametrize("d", [3, RES + 1])
def test_duplicates_far_rows_and_non_finite_values(gpu, d):
    a, b = table(70, d, False, 3, 0.0), table(2 * T + 5, d, False, 4, 0.0)
    b[7], b[40] = a[2], a[2]                                      # duplicates: k = 1 up to the bound, q clamped, never negative
    a[5] = np.sqrt(120.0 / d)                                      # far, q ~ 120 + d: k = 2^-(q / 2) is a normal number and 0 on the upper rungs
    want, bound = MR.kernel_sums(a, b, 0.5, 8, None, None, False, LIB.d3p_kernel_sums_roundings(70, 2 * T + 5))
    got = M.kernel_sums(dev(a, 1), dev(b), 0.5, 8)
    assert bool((np.abs(got.cpu().numpy() - want) <= bound).all()) and float(got[0, 2]) >= 2.0 - bound[0, 2] and float(got[7, 5]) == 0.0 < float(got[0, 5])
    clean = H.raw_bytes(got[:, :4])
    for word, in_b in ((NAN_WORD, False), (0x7f800000, False), (0xff800000, True), (0x7fc00000, True)):
        x = (b if in_b else a).copy()
        x.view(np.uint32)[4, d - 1] = word
        bad = M.kernel_sums(dev(x if not in_b else a), dev(x if in_b else b, 2), 0.5, 8)
        if in_b:
            assert bool(bad.isnan().all())
        else:
            assert bool(bad[:, 4].isnan().all()) and not bool(bad[:, :4].isnan().any()) and not bool(bad[:, 5:].isnan().any())
            assert torch.equal(H.raw_bytes(bad[:, :4]), clean)


def test_mmd_end_to_end_and_equal_tables(gpu):
    x, y = table(150, 4, False, 5), (table(90, 4, False, 6) * np.float32(1.0002)).astype(np.float32)
    xd, yd = dev(x, 1), dev(y, 2)
    got = M.mmd(xd, yd, n_bandwidths=3)
    mom = M.CV.column_moments(xd)
    shift, scale = mom.mean.float().cpu().numpy(), (1.0 / (mom.m2.diagonal() / 149.0).sqrt()).float().cpu().numpy()
    tx, ty = MR.transform(x, shift, scale).astype(np.float64), MR.transform(y, shift, scale).astype(np.float64)
    pooled = np.concatenate([tx, ty])
    q = ((pooled[:, None, :] - pooled[None, :, :]) ** 2).sum(axis=2)[np.triu_indices(240, 1)]
    centre = float(torch.tensor(q).median())                       # (torch's median: the lower of the two middle values)
    assert np.abs(got.sigma2.cpu().numpy() / (centre * 2.0 ** (1.0 - np.arange(3))) - 1.0).max() < 1e-9
    for b in range(3):
        s2 = 1.0 / (2.0 * np.log(2.0) * float(np.float32(1.0 / (2.0 * np.log(2.0) * float(got.sigma2[0])))) * 2 ** b)
        v, u, wx, wy = MR.mmd(tx, ty, s2)
        # a k errs by E_b ~ 2^b ln 2 gamma0 dq relative, dq <= 2 gamma_34 (ra + rb), (ra + rb) / (2 sigma2[0]) <= 8 here: 4 x 2 x 8 gamma_34
        tol = 64 * 34 * MR.U32
        assert abs(float(got.mmd2[b]) - v) <= 4 * tol and abs(float(got.mmd2_unbiased[b]) - u) <= 4 * tol
        assert np.abs(got.witness_x[b].cpu().numpy() - wx).max() <= 2 * tol and np.abs(got.witness_y[b].cpu().numpy() - wy).max() <= 2 * tol
    same = M.mmd(xd, dev(x), bandwidth=centre, n_bandwidths=3)
    assert float(same.mmd2.abs().max()) <= 4 * tol and float(same.witness_x.abs().max()) <= 2 * tol      # within the bound of 0, not 0 (module docstring)


def test_the_example_prints_one_line_per_bandwidth(gpu, capsys):
    spec = importlib.util.spec_from_file_location("ex_gmm_mmd", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples",
                                                                            "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["--mmd"]).mmd == 5 and mod.parse_args(["--mmd", "3"]).mmd == 3 and mod.parse_args([]).mmd is None
    mod.main(argparse.Namespace(num_epochs=2, learning_rate=5e-2, batch_size=64, dimensions=2, num_samples=512, num_components=3, sigma=0.3, mmd=3))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("MMD (sigma^2")]
    assert len(lines) == 3 and all("512 synthetic rows): MMD^2 " in ln and "unbiased" in ln and "largest witness" in ln for ln in lines)
