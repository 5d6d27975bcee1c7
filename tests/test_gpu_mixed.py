"""Mixed-type pair statistics on the GPU (d3p_pair_stats_mixed, d3p_amd.mixed) against tests/mixed_ref.py under each forced form and
both dtypes.  `min`, `argmin` and every flag BY VALUE (the inputs are of the class whose single final rounding is the kernel's: mixed_ref's
header); `sum` within gamma(k) * sum(dist) of math.fsum of the restated float32 distances, k = d3p_pair_stats_mixed_roundings(nb), u =
2^-53; the forms and the workspace's previous contents change no bit.  The largest error / bound is printed (docs/experiments_mixed.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

import d3p_amd._lib as L
from tests import mixed_ref as MR
from tests.test_mixed_host import SPLITS, kinds

pytestmark = pytest.mark.gpu
PAD = 64
_REF = {}      # case -> the restatement's outputs: computed once, shared by the forms, never changed


@pytest.fixture(scope="module")
def LIB(gpu):
    lib = L.load()
    yield lib
    assert lib.d3p_pair_stats_mixed_set_form(0) == 0


@pytest.fixture(params=(1, 2), ids=("wide-form", "split-form"))
def form(request, LIB):
    assert LIB.d3p_pair_stats_mixed_set_form(request.param) == 0
    yield request.param
    assert LIB.d3p_pair_stats_mixed_set_form(0) == 0


def entry(a, b, kind, scale, w_cat, excl=False, pads=(0, 0), fill=0xFF, short=0):
    """One call with a_ld = d + pads[0], b_ld = d + pads[1], 0xFF outputs between guards, the workspace filled with `fill`: (rc, outputs)."""
    lib = L.load()
    (na, d), nb, dc = a.shape, b.shape[0], int(sum(kind))
    tabs = []
    for t, pad in ((a, pads[0]), (b, pads[1])):
        buf = torch.full((t.shape[0], d + pad), 77, dtype=torch.int32 if a.dtype == np.int32 else torch.float32, device="cuda")
        buf[:, :d] = torch.tensor(t)
        tabs.append(buf)
    outs = [torch.full((PAD + na * w + PAD,), -1, dtype=torch.int32, device="cuda") for w in (2, 1, 1)]
    need = int(lib.d3p_pair_stats_mixed_workspace(na, nb, d - dc, dc))
    ws = torch.full((need + 8,), 0 if fill == "random" else fill, dtype=torch.uint8, device="cuda")
    if fill == "random":
        ws.random_(0, 256, generator=torch.Generator(device="cuda").manual_seed(9))
    guard = ws[need:].clone()
    k, s = (C.c_uint8 * d)(*kind), (C.c_float * d)(*[float(v) for v in scale])
    rc = lib.d3p_pair_stats_mixed(L.stream_ptr(), L.ptr(tabs[0]), L.ptr(tabs[1]), int(a.dtype == np.int32), d + pads[0], d + pads[1], na, nb, d,
                                  C.cast(k, C.c_void_p), C.cast(s, C.c_void_p), w_cat, int(excl), L.ptr(outs[0][PAD:]), L.ptr(outs[1][PAD:]),
                                  L.ptr(outs[2][PAD:]), L.ptr(ws), need - short)
    torch.cuda.synchronize()
    for o, w in zip(outs, (2, 1, 1)):
        assert bool((o[:PAD] == -1).all()) and bool((o[PAD + na * w:] == -1).all()), "an output was written outside its extent"
    assert torch.equal(ws[need:], guard), "the workspace was written outside its extent"
    if rc != 0:
        assert all(bool((o == -1).all()) for o in outs), "a refused call touched an output"
        return rc, None
    idx = outs[2][PAD:PAD + na].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return 0, {"sum": outs[0][PAD:PAD + 2 * na].contiguous().view(torch.float64).cpu().numpy().copy(),
               "min": outs[1][PAD:PAD + na].contiguous().view(torch.float32).cpu().numpy().copy(), "argmin": np.where(idx == 0xFFFFFFFF, -1, idx)}


def check(LIB, name, a, b, kind, scale, w, excl=False, **kw):
    """One call against the restatement: min, argmin and the flags by value, sum within its bound; returns (outputs, error / bound)."""
    if name not in _REF:
        _REF[name] = MR.emulate(a, b, kind, scale, w, excl)
    ref = _REF[name]
    rc, got = entry(a, b, kind, scale, w, excl, **kw)
    assert rc == 0, (name, rc, LIB.d3p_last_error())
    assert np.array_equal(got["min"], ref["min"], equal_nan=True) and np.array_equal(got["argmin"], ref["argmin"]), name
    assert np.array_equal(np.isnan(got["sum"]), np.isnan(ref["sum"])), name
    ok, mask = ~np.isnan(ref["sum"]), ~np.eye(*ref["dist"].shape, dtype=bool) if excl else np.ones(ref["dist"].shape, bool)
    tol = MR.gamma(int(LIB.d3p_pair_stats_mixed_roundings(b.shape[0])), MR.U64) * np.where(mask, ref["dist"].astype(np.float64), 0).sum(axis=1)
    err = np.abs(got["sum"] - ref["sum"])[ok]
    assert (err <= tol[ok]).all(), (name, float((err / tol[ok]).max()))
    return got, float((err[tol[ok] > 0] / tol[ok][tol[ok] > 0]).max()) if (tol[ok] > 0).any() else 0.0


@pytest.mark.parametrize("is_int", (False, True), ids=("float32", "int32"))
def test_against_the_restatement_at_every_edge(LIB, form, is_int):
    worst, cases = 0.0, [(na, nb, 3, 5, False, (0, 0)) for na in (1, 31, 32, 33, 65) for nb in (1, 31, 32, 33, 65)]
    cases += [(33, 65, dn, dc, False, (3, 1)) for dn, dc in SPLITS] + [(33, 513, 3, 5, False, (0, 2)), (65, 65, 4, 4, True, (1, 1)), (1, 1, 3, 5, True, (0, 0))]
    for na, nb, dn, dc, excl, pads in cases:
        kind = kinds(dn, dc)
        scale, w = MR.schema(5, kind)
        b = MR.data(2, nb, kind, is_int)
        a = MR.data(1, na, kind, is_int) if not excl else b
        if excl and na > 40:
            b[40], b[7] = b[3], b[33]                                       # duplicate rows on both sides of a tile edge
        _, r = check(LIB, (na, nb, dn, dc, excl, is_int), a, b, kind, scale, w, excl, pads=pads)
        worst = max(worst, r)
    print(f"form {form} {'int32' if is_int else 'float32'}: largest sum error / bound {worst:.3f}")


def test_all_categorical_ties_and_codes_beside_pad_bytes(LIB, form):
    """dist = w_cat m is exact: many ties, each to the smallest j; dc = 5 and 129 leave 3 pad bytes beside the codes 0 and 255."""
    for dc in (1, 5, 129):
        rng = np.random.default_rng(dc)
        a, b = (np.array([0, 255])[rng.integers(0, 2, (n, dc))].astype(np.float32) for n in (33, 70))
        b[37], b[64], b[5] = b[2], b[2], a[9]
        got, _ = check(LIB, ("cat", dc), a, b, [1] * dc, np.zeros(dc, np.float32), 0.75)
        m = (a[:, None, :] != b[None, :, :]).sum(axis=2)
        assert np.array_equal(got["min"], (0.75 * m.min(axis=1)).astype(np.float32)) and np.array_equal(got["argmin"], m.argmin(axis=1))
        assert np.array_equal(got["sum"], 0.75 * m.sum(axis=1)) and got["min"][9] == 0.0           # (multiples of 0.25 below 2^53: exact)


def test_special_rows_and_the_workspace(LIB, form):
    kind = kinds(3, 5)
    num, cat = kind.index(0), kind.index(1)
    scale, w = MR.schema(5, kind)
    a, b = MR.data(1, 40, kind, False), MR.data(2, 70, kind, False)
    a[2, num], a[5, cat], a[33, cat], a[34, cat], a[35, cat] = np.nan, 256, -1, 0.5, -0.0
    got, _ = check(LIB, "special a", a, b, kind, scale, w)
    assert np.nonzero(np.isnan(got["min"]))[0].tolist() == [2, 5, 33, 34] and (got["argmin"][[2, 5, 33, 34]] == -1).all()
    bits = lambda out: tuple(np.ascontiguousarray(out[k]).tobytes() for k in ("sum", "min", "argmin"))  # noqa: E731
    base = bits(got)
    for fill in (0x00, "random"):                                            # what the workspace held changes no bit
        assert bits(entry(a, b, kind, scale, w, fill=fill)[1]) == base
    assert LIB.d3p_pair_stats_mixed_set_form(3 - form) == 0                  # nor does the form
    assert bits(entry(a, b, kind, scale, w)[1]) == base
    assert entry(a, b, kind, scale, w, short=1)[0] == -4 and b"workspace too small" in LIB.d3p_last_error()
    for bad in (np.inf, 256.0):
        b2 = b.copy()
        b2[69, num if bad == np.inf else cat] = bad
        got, _ = check(LIB, ("special b", bad), a, b2, kind, scale, w)
        assert np.isnan(got["sum"]).all() and np.isnan(got["min"]).all() and (got["argmin"] == -1).all()


def test_python_layer(gpu):
    from d3p_amd import fidelity as F
    from d3p_amd import mixed as M
    rng = np.random.default_rng(3)
    real = np.concatenate([rng.normal(size=(300, 3)), rng.integers(0, 4, (300, 2))], axis=1).astype(np.float32)
    real[:, 0] += 3.0 * real[:, 3]                                           # the first category moves a numeric column
    x = torch.tensor(real, device="cuda")
    schema = M.mixed_schema(x, (3, 4))
    assert schema.kind == (0, 0, 0, 1, 1) and schema.total_weight == 5.0 and schema.w_cat == 1.0
    assert schema.scale[:3] == tuple(float(np.float32(1.0 / (real[:, c].astype(np.float64).max() - real[:, c].astype(np.float64).min()))) for c in range(3))
    out = M.pair_stats(x[:50], x, schema)
    g = MR.exact(real[:50], real, schema.kind, np.array(schema.scale, np.float32), schema.w_cat)["sum"] / 5.0
    assert np.allclose(out["sum"].cpu().numpy(), g, rtol=1e-5) and not out["min"].any()
    assert out["argmin"].cpu().tolist() == list(range(50)) and out["min"].dtype == torch.float64
    assert float(M.energy_distance(x, x, schema).d2) == 0.0
    synth = x.clone()
    synth[:, 3] = x[torch.randperm(300, generator=torch.Generator().manual_seed(1)).cuda(), 3]   # a copy but for one permuted categorical column
    e = M.energy_distance(synth, x, schema)
    assert float(e.d2) > 0.0 and (M.closest_record(synth, x, schema)["distance"] <= 1.0 / 5.0 + 1e-12).all()
    r = F.fidelity_report(x, synth, schema=schema)
    assert float(r.energy_train.d2) == float(e.d2) and r.n_exact_copies == int((synth[:, 3] == x[:, 3]).sum())
    plain, none = F.fidelity_report(x, synth), F.fidelity_report(x, synth, schema=None)
    assert all(torch.equal(p, q) if isinstance(p, torch.Tensor) else p == q for p, q in zip(plain.energy_train, none.energy_train))
    assert plain[2:] == none[2:]
