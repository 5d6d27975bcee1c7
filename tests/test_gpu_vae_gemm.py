"""The VAE's product kernels (d3p_amd/csrc/d3p_gemm.hip: k_gemm_f32, k_gemm_f32_w8, k_gemm_bf16x3, k_gemm_bf16x3_group,
k_gemm_reduce) one option at a time, through the test aids d3p_gemm_f32_ex / d3p_gemm_f32_group, against the float64 restatement
of tests/vae_gemm_ref.py.

Every case asserts the route the dispatcher REPORTS before it looks at numbers, every output lies in a buffer with a canary border
(C with ldc > N, the split tiles, the row sums of epilogue 4) that is checked after the call.

Tolerances: products -- the project's figures (vae_gemm_ref.TOL_F32 = 2e-5 of max sum_k |a||b| for the fp32 kernels and the
2048-deep product, TOL_BF16 = 3e-6 of each element's sum_k |a||b| for the bf16x3 kernel at K <= 1024; a bias and an accumulated C
add their magnitude to the element's scale: the final fma rounds at that size).  Identities -- torch.equal.  Epilogues -- four
times the worst error of the float32 torch restatement of the formula on the same inputs (vae_gemm_ref.epi_bounds); the device's
worst ratio to that bound is printed per case and recorded in docs/experiments_vae_gemm.md."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_gemm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 1234.5
BORDER = 64        # floats on either side of every output (a multiple of 4: the inside stays 16-byte aligned)
F32, F32_VA, F32_VB, W8, BF16, GROUPED = 0, 1, 2, 4, 5, 6


@pytest.fixture(scope="module")
def lib(gpu):
    import d3p_amd._lib as L
    return L


class Boxed:
    """n floats between two canary borders."""

    def __init__(self, n, fill=CANARY):
        self.buf = torch.full((n + 2 * BORDER,), CANARY, device="cuda")
        self.x = self.buf[BORDER:BORDER + n]
        self.x.fill_(fill)

    def borders_intact(self):
        return bool((self.buf[:BORDER] == CANARY).all()) and bool((self.buf[-BORDER:] == CANARY).all())


def make_operands(form, M, N, K, seed, a_last_one=False, big=True, lda=None, ldb=None, A=None, Bm=None, pad=None):
    """Storage of op(A) (the M - 1 rows in memory when a_last_one) and op(B) in an operand form, row strides rounded up to 4 for the
    eight-wave kernels; the padding inside the row strides holds randn (junk that must not leak), or `pad`."""
    g = torch.Generator().manual_seed(seed)
    m_real = M - 1 if a_last_one else M
    A = torch.randn(m_real, K, generator=g) if A is None else A
    Bm = torch.randn(K, N, generator=g) if Bm is None else Bm
    if lda is None:
        lda = (R.rup4(K) if form[0] == "n" else R.rup4(m_real)) if big else (K if form[0] == "n" else m_real)
    if ldb is None:
        ldb = (R.rup4(N) if form[1] == "n" else R.rup4(K)) if big else (N if form[1] == "n" else K)

    def store(dense, ld):     # dense [rows, fast] -> [rows, ld]
        s = torch.randn(dense.shape[0], ld, generator=g) if pad is None else torch.full((dense.shape[0], ld), float(pad))
        s[:, :dense.shape[1]] = dense
        return s.cuda()
    a_t = store(A if form[0] == "n" else A.t(), lda)
    b_t = store(Bm if form[1] == "n" else Bm.t(), ldb)
    a_sm, a_sk = (lda, 1) if form[0] == "n" else (1, lda)
    b_sk, b_sn = (ldb, 1) if form[1] == "n" else (1, ldb)
    return dict(a=a_t, a_sm=a_sm, a_sk=a_sk, b=b_t, b_sk=b_sk, b_sn=b_sn, M=M, N=N, K=K, a_last_one=a_last_one)


def run(lib, op, bias=None, alpha=1.0, C0=None, ldc=None, jumps=None, part_splits=0, c_fill=CANARY, width=None, **kw):
    """One d3p_gemm_f32_ex call.  C is M x ldc (ldc = N + 3 unless given) between canary borders; C0 (accumulate) is scattered into
    the product's columns first.  part_splits > 0: split scratch of part_splits M N floats between borders.  Returns the product's
    columns of C, the report, and the buffers; asserts the borders and every column of C the product does not own."""
    M, N, K = op["M"], op["N"], op["K"]
    ldc = N + 3 if ldc is None else ldc
    cols = R.c_columns(N, jumps).cuda()
    own = cols if width is None else torch.cat([cols, cols + width])     # (epilogue 3 owns [dz | du])
    cbox = Boxed(M * ldc, c_fill)
    Cv = cbox.x.view(M, ldc)
    if C0 is not None:
        Cv[:, cols] = C0.cuda()
    o = lib.GemmOpts()
    o.a_last_one = int(op["a_last_one"])
    pbox = None
    if part_splits:
        pbox = Boxed(part_splits * M * N)
        o.part, o.part_floats = pbox.x.data_ptr(), part_splits * M * N
    if jumps is not None:
        o.has_jumps = 1
        for k, v in jumps.items():
            setattr(o, k, v)
    keep = []
    for k, v in kw.items():
        if torch.is_tensor(v):
            keep.append(v)
            v = v.data_ptr()
        setattr(o, k, v)
    rep = lib.GemmReport()
    L = lib.load()
    lib.check(L.d3p_gemm_f32_ex(lib.stream_ptr(), lib.ptr(op["a"]), op["a_sm"], op["a_sk"], lib.ptr(op["b"]), op["b_sk"], op["b_sn"],
                                C.c_void_p(cbox.x.data_ptr()), ldc, M, N, K, lib.ptr(bias), alpha, int(C0 is not None), C.byref(o), C.byref(rep)))
    torch.cuda.synchronize()
    assert cbox.borders_intact(), "C: border overwritten"
    other = torch.ones(ldc, dtype=torch.bool, device="cuda")
    other[own] = False
    assert bool((Cv[:, other] == c_fill).all()), "C: a column outside the product overwritten"
    if pbox is not None:
        assert pbox.borders_intact(), "part: border overwritten"
    return dict(C=Cv[:, cols].clone(), Cfull=Cv, rep=rep, part=None if pbox is None else pbox.x, route=rep.route, splits=rep.splits, left=rep.splits_left)


def reference(op, bias=None, alpha=1.0, C0=None, jumps=None):
    A, B = R.operands(op["a"], op["a_sm"], op["a_sk"], op["b"], op["b_sk"], op["b_sn"], op["M"], op["N"], op["K"], op["a_last_one"], jumps)
    ref, scale = R.product(A, B, bias, alpha, C0)
    scale = abs(alpha) * scale
    if bias is not None:
        scale = scale + bias.detach().cpu().double().abs().view(1, -1)
    if C0 is not None:
        scale = scale + C0.detach().cpu().double().abs()
    return ref, scale


def assert_product(out, ref, scale, route, K):
    err = (out.double().cpu() - ref).abs()
    assert bool(torch.isfinite(out).all())
    if route in (BF16, GROUPED) and K <= 1024:
        worst = float((err / scale.clamp_min(1e-300)).max())
        assert worst <= R.TOL_BF16, worst
    else:
        assert float(err.max()) <= R.TOL_F32 * float(scale.max()), (float(err.max()), float(scale.max()))


def tile_sum(part, splits, M, N):
    """The tiles summed in float32 in slab order, as k_gemm_reduce and k_vae_tile_sums sum them."""
    t = part[:splits * M * N].view(splits, M, N)
    s = torch.zeros(M, N, device="cuda")
    for z in range(splits):
        s = s + t[z]
    return s


# ---- plain product ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("M,N,K", R.BIG_SHAPES)
def test_plain_product_bf16(lib, M, N, K, form):
    op = make_operands(form, M, N, K, M + N + K)
    g = torch.Generator().manual_seed(K)
    bias, C0 = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g)
    r = run(lib, op, bias=bias, alpha=0.5, C0=C0)
    assert (r["route"], r["splits"], r["left"]) == (BF16, 1, 0)
    assert_product(r["C"], *reference(op, bias, 0.5, C0), r["route"], K)
    r = run(lib, op)
    assert r["route"] == BF16
    assert_product(r["C"], *reference(op), r["route"], K)


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("M,N,K", R.F32_SHAPES)
def test_plain_product_f32(lib, M, N, K, form):
    op = make_operands(form, M, N, K, M + N + K, big=False)
    g = torch.Generator().manual_seed(K)
    bias, C0 = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g)
    r = run(lib, op, bias=bias, alpha=0.5, C0=C0)
    assert (r["route"], r["splits"]) == (R.f32_route(form, M, N, K), 1)
    assert_product(r["C"], *reference(op, bias, 0.5, C0), r["route"], K)
    r = run(lib, op)
    assert_product(r["C"], *reference(op), r["route"], K)


# ---- split-K ---------------------------------------------------------------------------------------------------------------------
def _split_checks(lib, op, want_route, want_splits, **kw):
    M, N, K = op["M"], op["N"], op["K"]
    g = torch.Generator().manual_seed(K + 1)
    bias, C0 = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g)
    red = run(lib, op, part_splits=want_splits, **kw)
    assert (red["route"], red["splits"], red["left"]) == (want_route, want_splits, 0)
    assert_product(red["C"], *reference(op), red["route"], K)
    left = run(lib, op, part_splits=want_splits, leave_split=1, **kw)
    assert (left["route"], left["splits"], left["left"]) == (want_route, want_splits, want_splits)
    assert bool((left["Cfull"] == CANARY).all()), "tiles left: C must not be written"
    s = tile_sum(left["part"], want_splits, M, N)
    assert torch.equal(s, red["C"])                                  # fma(1, s, 0) = s
    assert torch.equal(red["part"], left["part"])
    # bias, alpha != 1 (one fma: restated in float64, rounded once) and accumulate (one more float32 add)
    full = run(lib, op, bias=bias, alpha=0.75, C0=C0, part_splits=want_splits, **kw)
    assert (full["route"], full["splits"]) == (want_route, want_splits)
    want = R.fma_round(0.75, s.cpu(), bias.cpu().view(1, -1).expand(M, N)) + C0
    assert torch.equal(full["C"].cpu(), want)
    assert_product(full["C"], *reference(op, bias, 0.75, C0), full["route"], K)


@pytest.mark.parametrize("form", ["nn", "tn", "nt"])
@pytest.mark.parametrize("M,N,K,sp", R.BIG_SPLITS)
def test_split_product_bf16(lib, M, N, K, sp, form):
    assert R.split_count_ok(sp, K)[0]
    _split_checks(lib, make_operands(form, M, N, K, M + N + K + sp), BF16, sp, force_splits=sp)


@pytest.mark.parametrize("form", ["nn", "tt"])
@pytest.mark.parametrize("M,N,K", R.F32_SPLITS)
def test_split_product_f32(lib, M, N, K, form):
    sp = R.f32_split_count(M, N, K)
    assert sp > 1
    _split_checks(lib, make_operands(form, M, N, K, M + N + K, big=False), R.f32_route(form, M, N, K), sp)


def test_split_product_bf16_by_part_alone(lib):
    """`part` without force_splits: the dispatcher's own count for a short grid (2 tiles, K = 200 -> four slabs of 64 on any chip of
    eight or more compute units: rounds of one, the cost is the K range alone)."""
    op = make_operands("nn", 129, 64, 200, 5)
    r = run(lib, op, part_splits=16)
    assert (r["route"], r["splits"]) == (BF16, 4)
    assert_product(r["C"], *reference(op), r["route"], 200)


# ---- a_last_one --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [True, False])
@pytest.mark.parametrize("form", ["nn", "tn"])
@pytest.mark.parametrize("rem", [0, 1, 2, 3])
def test_virtual_row_of_ones_equals_the_row_in_memory(lib, rem, form, big):
    m_real = (128 if big else 60) + rem           # M - 1 = 0 .. 3 (mod 4)
    M, N, K = m_real + 1, 68 if big else 65, 100 if big else 16
    lda = R.rup4(M) + 4 if form == "tn" else R.rup4(K)      # (m-fast: a stride beyond roundup4(M - 1), and room for the row in memory)
    g = torch.Generator().manual_seed(rem)
    A = torch.randn(m_real, K, generator=g)
    virt = make_operands(form, M, N, K, 11, a_last_one=True, big=big, lda=lda, A=A)
    mem = make_operands(form, M, N, K, 11, a_last_one=False, big=big, lda=lda, A=torch.cat([A, torch.ones(1, K)]), Bm=R.strided(virt["b"], K, N, virt["b_sk"], virt["b_sn"]).float())
    rv, rm = run(lib, virt), run(lib, mem)
    assert rv["route"] == rm["route"] == (BF16 if big else R.f32_route(form, lda if form == "tn" else M, N, K))
    assert torch.equal(rv["C"], rm["C"])
    assert_product(rv["C"], *reference(virt), rv["route"], K)
    if big:   # ... and through split tiles
        rv, rm = run(lib, virt, part_splits=2, force_splits=2, leave_split=1), run(lib, mem, part_splits=2, force_splits=2, leave_split=1)
        assert rv["left"] == rm["left"] == 2 and torch.equal(rv["part"], rm["part"])


def test_virtual_row_of_ones_that_changes_the_route(lib):
    """M - 1 = 96 rows in memory: with the row of ones M = 97 takes the bf16 kernel, the 96 rows alone the 64 x 64 kernel -- the
    products agree at the tolerance."""
    M, N, K = 97, 68, 100
    virt = make_operands("nn", M, N, K, 3, a_last_one=True)
    rv = run(lib, virt)
    assert rv["route"] == BF16
    body = dict(virt, M=M - 1, a_last_one=False)
    rb = run(lib, body)
    assert rb["route"] == (F32 | F32_VA | F32_VB)
    ref, scale = reference(virt)
    assert_product(rv["C"], ref, scale, BF16, K)
    assert_product(rb["C"], ref[:M - 1], scale[:M - 1], rb["route"], K)


# ---- displaced segments ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,n_seg,k_seg", [(129, 100, 50, 50, 30), (129, 100, 50, 64, 25), (129, 100, 50, 37, 50), (65, 100, 17, 50, 9), (65, 100, 16, 50, 9), (5, 6, 3, 3, 2), (63, 130, 70, 64, 16)])
def test_displaced_segments(lib, M, N, K, n_seg, k_seg):
    """B, the bias and C in two segments each, every jump different: one jump used for another moves data.  A displaced B is fetched by
    the 64 x 64 kernel's scalar path (VB off), whatever M."""
    jumps = dict(n_seg=n_seg, k_seg=k_seg, b_njump=7 * N + 5, b_kjump=3 * N + 1, bias_njump=11, c_njump=4)
    g = torch.Generator().manual_seed(M + n_seg)
    a = torch.randn(M, K, generator=g).cuda()
    b = torch.randn(K * N + jumps["b_njump"] + jumps["b_kjump"] + N, generator=g).cuda()
    bias = torch.randn(N + jumps["bias_njump"], generator=g).cuda()
    op = dict(a=a, a_sm=K, a_sk=1, b=b, b_sk=N, b_sn=1, M=M, N=N, K=K, a_last_one=False)
    r = run(lib, op, bias=bias, jumps=jumps, ldc=N + 9)
    assert r["route"] == (F32 | (F32_VA if K % 4 == 0 else 0))
    A, B = R.operands(a, K, 1, b, N, 1, M, N, K, False, jumps)
    ref, scale = R.product(A, B, R.gather_bias(bias, N, jumps))
    assert_product(r["C"], ref, scale + R.gather_bias(bias, N, jumps).double().abs().view(1, -1), r["route"], K)


@pytest.mark.parametrize("split", [0, 3])
def test_displaced_bias_and_output_on_the_bf16_kernel(lib, split):
    """The heads' weight gradient: C's second half displaced (and, for the packed heads' forward product, the bias's), B plain."""
    M, N, K = 129, 100, 200
    jumps = dict(n_seg=50, k_seg=0x7fffffff, b_njump=0, b_kjump=0, bias_njump=13, c_njump=6)
    op = make_operands("tn", M, N, K, 21, a_last_one=True)
    bias = torch.randn(N + 13, generator=torch.Generator().manual_seed(2)).cuda()
    r = run(lib, op, bias=bias, jumps=jumps, ldc=N + 11, part_splits=split, force_splits=split)
    assert (r["route"], r["splits"]) == (BF16, max(split, 1))
    bg = R.gather_bias(bias, N, jumps)
    ref, scale = reference(op, bg)
    assert_product(r["C"], ref, scale, BF16, K)


# ---- epilogues 1 - 3 -----------------------------------------------------------------------------------------------------------
RATIOS = {}     # worst device error / bound per epilogue output, printed by the last epilogue test (docs/experiments_vae_gemm.md)


def _epi_compare(name, outs, o_dev, *ops):
    ref = R.epi_outputs(name, o_dev.cpu(), *ops)
    errs = R.rel_errors([t.cpu() for t in outs], ref, R.epi_scales(name, o_dev.cpu(), *ops))
    bounds = R.epi_bounds(name, o_dev.cpu(), *ops)
    for i, (e, b) in enumerate(zip(errs, bounds)):
        key = f"{name}[{i}]"
        RATIOS[key] = max(RATIOS.get(key, 0.0), e / b if b > 0 else (0.0 if e == 0 else float("inf")))
        print(f"{key}: device error {e:.3e}, bound {b:.3e}")
    for e, b in zip(errs, bounds):
        assert e <= b, (name, errs, bounds)


EPI_ROUTES = [("bf16", 129, 100, 200, 0), ("bf16", 260, 68, 50, 0), ("bf16-split", 129, 132, 200, 3), ("f32", 65, 130, 17, 0), ("f32", 64, 64, 16, 0),
              ("f32-split", 65, 68, 200, 0)]
SPECIAL = [0.0, -0.0, 20.0, -20.0, 90.0, -90.0, float("inf")]


def _epi_setup(kind, M, N, K, sp, form="nn", Bm=None):
    big = kind.startswith("bf16")
    op = make_operands(form, M, N, K, M + K, big=big, Bm=Bm)
    kw = dict(part_splits=(sp if big else R.f32_split_count(M, N, K)) if "split" in kind else 0)
    if big and sp:
        kw["force_splits"] = sp
    want = (BF16 if big else R.f32_route(form, M, N, K), max(kw["part_splits"], 1))
    return op, kw, want


@pytest.mark.parametrize("kind,M,N,K,sp", EPI_ROUTES)
def test_epilogue_1_softplus_and_sigmoid(lib, kind, M, N, K, sp):
    # columns 0 .. 6 of B are zero: the accumulator is +0 and o = fma(1, 0, bias) = the bias exactly (0, -0, +-20, +-90, +Inf)
    Bm = torch.randn(K, N, generator=torch.Generator().manual_seed(5))
    Bm[:, :len(SPECIAL)] = 0.0
    op, kw, want = _epi_setup(kind, M, N, K, sp, Bm=Bm)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(4))
    bias[:len(SPECIAL)] = torch.tensor(SPECIAL)
    bias = bias.cuda()
    plain = run(lib, op, bias=bias, **kw)
    assert (plain["route"], plain["splits"]) == want
    o_dev = plain["C"]
    assert torch.equal(o_dev[:, :len(SPECIAL)].cpu(), torch.tensor(SPECIAL).view(1, -1).expand(M, -1))
    c2 = Boxed(M * (N + 3))
    r = run(lib, op, bias=bias, epi=1, C2=c2.x, **kw)
    assert (r["route"], r["splits"]) == want
    sig = c2.x.view(M, N + 3)
    assert c2.borders_intact() and bool((sig[:, N:] == CANARY).all())
    _epi_compare("epi1", [r["C"], sig[:, :N]], o_dev)      # (C2 is the sigmoid)


@pytest.mark.parametrize("kind,M,N,K,sp", EPI_ROUTES)
def test_epilogue_2_times_c2(lib, kind, M, N, K, sp):
    op, kw, want = _epi_setup(kind, M, N, K, sp, form="nt")      # (the backward-data products: B k-fast)
    plain = run(lib, op, **kw)
    assert (plain["route"], plain["splits"]) == want
    c2 = Boxed(M * (N + 3))
    c2v = c2.x.view(M, N + 3)
    c2v[:, :N] = torch.rand(M, N, generator=torch.Generator().manual_seed(6)).cuda()
    before = c2.buf.clone()
    r = run(lib, op, epi=2, C2=c2.x, **kw)
    assert (r["route"], r["splits"]) == want
    assert torch.equal(c2.buf, before), "epilogue 2 only reads C2"
    _epi_compare("epi2", [r["C"]], plain["C"], c2v[:, :N].cpu())


@pytest.mark.parametrize("Z", [1, 3, 50])
@pytest.mark.parametrize("kind,M,K,sp", [("bf16", 129, 100, 0), ("bf16-split", 260, 200, 3), ("f32", 65, 17, 0), ("f32-split", 5, 200, 0)])
def test_epilogue_3_latent_backward(lib, kind, M, K, sp, Z):
    op, kw, want = _epi_setup(kind, M, Z, K, sp, form="nt")      # (the dz product: A = delta, B = V1 read k-fast)
    ldc, sc = 2 * Z + 3, 0.75
    plain = run(lib, op, ldc=ldc, **kw)
    assert (plain["route"], plain["splits"]) == want
    g = torch.Generator().manual_seed(Z)
    zu = Boxed(M * ldc)
    zuv = zu.x.view(M, ldc)
    zuv[:, :2 * Z] = torch.cat([torch.randn(M, Z, generator=g), torch.rand(M, Z, generator=g) + 0.1], 1).cuda()
    eps = torch.randn(M, Z, generator=g).cuda()
    before = zu.buf.clone()
    r = run(lib, op, ldc=ldc, width=Z, epi=3, ex_zu=zu.x, ex_eps=eps, ex_Z=Z, ex_sc=sc, **kw)
    assert (r["route"], r["splits"]) == want
    assert torch.equal(zu.buf, before), "ex_zu is read only"
    _epi_compare("epi3", [r["Cfull"][:, :Z], r["Cfull"][:, Z:2 * Z]], plain["C"], zuv[:, :Z].cpu(), zuv[:, Z:2 * Z].cpu(), eps.cpu(), sc)


# ---- epilogue 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [129, 260])
@pytest.mark.parametrize("N", [68, 100, 132])
def test_epilogue_4_output_layer(lib, M, N):
    K, sc = 50, 1.25
    op = make_operands("nn", M, N, K, M + N)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(8)).cuda()
    plain = run(lib, op, bias=bias)
    assert plain["route"] == BF16
    G = -(-N // 32)
    xb = Boxed(M * (N + 3), 0.0)
    xv = xb.x.view(M, N + 3)
    xv[:, :N] = torch.rand(M, N, generator=torch.Generator().manual_seed(9)).cuda()
    ll, xx = Boxed(G * M), Boxed(G * M)
    r = run(lib, op, bias=bias, epi=4, ex_sc=sc, ep_x=xb.x, ep_ll=ll.x, ep_xx=xx.x)
    assert (r["route"], r["splits"]) == (BF16, 1)
    assert ll.borders_intact() and xx.borders_intact(), "a group of columns beyond ceil(N / 32) written"
    _epi_compare("epi4", [r["C"], ll.x.view(G, M), xx.x.view(G, M)], plain["C"], xv[:, :N].cpu(), sc)


def test_epilogue_4_refusals(lib):
    for M, split in ((129, 2), (64, 0)):      # a split product; one that does not take the bf16 kernel
        op = make_operands("nn", M, 68, 200, 1)
        x, ll, xx = torch.zeros(M, 71, device="cuda"), Boxed(3 * M), Boxed(3 * M)
        with pytest.raises(ValueError):
            run(lib, op, epi=4, ex_sc=1.0, ep_x=x, ep_ll=ll.x, ep_xx=xx.x, part_splits=split, force_splits=split)
        assert bool((ll.x == CANARY).all())
    op = make_operands("nt", 129, 68, 200, 1)     # a k-fast B
    with pytest.raises(ValueError):
        run(lib, op, epi=4, ex_sc=1.0, ep_x=torch.zeros(129, 71, device="cuda"), ep_ll=Boxed(3 * 129).x, ep_xx=Boxed(3 * 129).x)


def test_entry_refusals(lib):
    op = make_operands("nn", 129, 68, 200, 1)
    with pytest.raises(ValueError):
        run(lib, op, epi=1)                                       # C2 missing
    with pytest.raises(ValueError):
        run(lib, op, part_splits=2, force_splits=5)               # 200 in 5 slabs: the rounded range gives 4
    with pytest.raises(ValueError):
        run(lib, op, force_splits=2)                              # no part
    with pytest.raises(ValueError):
        run(lib, make_operands("nn", 129, 68, 64, 1), part_splits=2, force_splits=2)     # a range of one slice
    o = lib.GemmOpts()
    part = torch.zeros(129 * 68, device="cuda")
    o.part, o.part_floats = part.data_ptr(), 129 * 68 - 1        # smaller than M N
    rep, out = lib.GemmReport(), torch.zeros(129, 68, device="cuda")
    rc = lib.load().d3p_gemm_f32_ex(lib.stream_ptr(), lib.ptr(op["a"]), 200, 1, lib.ptr(op["b"]), 68, 1, lib.ptr(out), 68, 129, 68, 200, None, 1.0, 0, C.byref(o), C.byref(rep))
    assert rc == -1
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):                               # an A with padded rows is not contiguous
        run(lib, make_operands("nn", 129, 68, 50, 1), exact16_word=word, exact16_nonce=5)
    assert int(word) == 0


# ---- the one-plane route -------------------------------------------------------------------------------------------------------
NONCE = 0x5eed1234


@pytest.mark.parametrize("form,a_last_one", [("nn", False), ("tn", False), ("tn", True), ("nn", True)])
@pytest.mark.parametrize("kind", ["binary", "integers"])
def test_one_plane_route_equals_the_general_route(lib, kind, form, a_last_one):
    M, N, K = (129 if a_last_one else 128), 68, 100      # (128 rows in memory: contiguous in both forms)
    g = torch.Generator().manual_seed(3)
    A = (torch.rand(128, K, generator=g) < 0.3).float() if kind == "binary" else torch.randint(-100, 101, (128, K), generator=g).float()
    op = make_operands(form, M, N, K, 17, a_last_one=a_last_one, A=A)
    general = run(lib, op)
    assert general["route"] == BF16
    for preload, exact in ((0, True), (NONCE, False)):      # a stale match sends the exact batch down the general path: still right
        word = torch.full((1,), preload, dtype=torch.int32, device="cuda")
        r = run(lib, op, exact16_word=word, exact16_nonce=NONCE)
        assert r["route"] == BF16
        assert (int(word) != NONCE) == exact
        assert torch.equal(r["C"], general["C"])
    assert_product(general["C"], *reference(op), BF16, K)
    if a_last_one:      # ... and as the weight gradients run it: split tiles, the rows of B scaled
        sc = torch.rand(K, generator=g).cuda()
        kw = dict(part_splits=2, force_splits=2, leave_split=1, b_row_scale=sc)
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        a, b = run(lib, op, **kw), run(lib, op, exact16_word=word, exact16_nonce=NONCE, **kw)
        assert int(word) != NONCE and torch.equal(a["part"], b["part"])


@pytest.mark.parametrize("form", ["nn", "tn"])
@pytest.mark.parametrize("where", ["first", "last"])
def test_one_inexact_element_takes_the_general_route(lib, where, form):
    """One element of A with low bits, in the first or in the last 16-byte word the pass reads: the word must hold the nonce and the
    product must be fp32-accurate (one plane alone would miss that element's products by 2^-8)."""
    M, N, K = 128, 68, 100
    g = torch.Generator().manual_seed(4)
    A = (torch.rand(M, K, generator=g) < 0.3).float()
    op = make_operands(form, M, N, K, 19, A=A)
    flat = op["a"].view(-1)
    flat[0 if where == "first" else flat.numel() - 1] = 1.0 + 2.0 ** -10 + 2.0 ** -20
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    r = run(lib, op, exact16_word=word, exact16_nonce=NONCE)
    assert r["route"] == BF16 and int(word) == NONCE
    assert_product(r["C"], *reference(op), BF16, K)


# ---- b_row_scale ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,a_last_one", [("nn", False), ("tn", False), ("tn", True)])
@pytest.mark.parametrize("M,N,K,sp", [(129, 68, 50, 0), (260, 100, 33, 0), (129, 132, 200, 3), (97, 64, 100, 2), (128, 4, 1, 0)])
def test_row_scale_equals_prescaled_rows(lib, M, N, K, sp, form, a_last_one):
    op = make_operands(form, M, N, K, M + K, a_last_one=a_last_one)
    sc = torch.rand(K, generator=torch.Generator().manual_seed(K))
    sc[0] = 0.0
    sc[K // 2] = 1.0
    sc[K - 1] = 2.0 ** -20
    sc = sc.cuda()
    pre = dict(op, b=op["b"] * sc.view(-1, 1))                      # float32 products, rounded once, written to memory
    kw = dict(part_splits=sp, force_splits=sp)
    a, b = run(lib, op, b_row_scale=sc, **kw), run(lib, pre, **kw)
    assert a["route"] == b["route"] == BF16 and a["splits"] == b["splits"] == max(sp, 1)
    assert torch.equal(a["C"], b["C"])
    assert_product(a["C"], *reference(pre), BF16, K)
    if sp:
        a, b = run(lib, op, b_row_scale=sc, leave_split=1, **kw), run(lib, pre, leave_split=1, **kw)
        assert a["left"] == sp and torch.equal(a["part"], b["part"])


def test_row_scale_refused_off_the_bf16_kernel(lib):
    sc = torch.ones(16, device="cuda")
    with pytest.raises(ValueError):
        run(lib, make_operands("nn", 64, 64, 16, 1, big=False), b_row_scale=sc)
    with pytest.raises(ValueError):
        run(lib, make_operands("nt", 129, 64, 16, 1), b_row_scale=sc)      # a k-fast B


# ---- grouped launch ------------------------------------------------------------------------------------------------------------
def _member(lib, op, cbox, ldc, pbox, sp, scale=None, jumps=None):
    m = lib.GemmMember()
    m.A, m.a_sm, m.a_sk, m.B, m.b_sk, m.b_sn = op["a"].data_ptr(), op["a_sm"], op["a_sk"], op["b"].data_ptr(), op["b_sk"], op["b_sn"]
    m.C, m.ldc, m.M, m.N, m.K, m.alpha = cbox.x.data_ptr(), ldc, op["M"], op["N"], op["K"], 1.0
    m.opts.a_last_one, m.opts.leave_split = int(op["a_last_one"]), 1
    m.opts.part, m.opts.part_floats = pbox.x.data_ptr(), pbox.x.numel()
    if scale is not None:
        m.opts.b_row_scale = scale.data_ptr()
    if jumps is not None:
        m.opts.has_jumps = 1
        for k, v in jumps.items():
            setattr(m.opts, k, v)
    return m


def _run_group(lib, name, extra=None, sum_n=0):
    """The members of vae_gemm_ref.GROUPS[name] (the weight-gradient form: A m-fast with the row of ones, B n-fast; odd members with
    row scales, the last of three or more with a displaced half of C) in one grouped launch; every member alone with the same
    force_splits as the reference.  Returns per member (joined, tiles or C of the group, tiles or C alone)."""
    spec = R.GROUPS[name]
    K, sp = spec["K"], spec["splits"]
    sc = torch.rand(K, generator=torch.Generator().manual_seed(1)).cuda()
    ops, extras = [], []
    for i, (M, N) in enumerate(spec["members"]):
        jumps = dict(n_seg=N // 2, k_seg=0x7fffffff, b_njump=0, b_kjump=0, bias_njump=0, c_njump=5) if (i == len(spec["members"]) - 1 and i >= 2 and N >= 8) else None
        ops.append((make_operands("tn", M, N, K, 100 + i, a_last_one=True), sc if i % 2 else None, jumps))
    if extra is not None:
        ops.insert(1, extra)
    Ms = (lib.GemmMember * len(ops))()
    boxes = []
    for i, (op, scale, jumps) in enumerate(ops):
        ldc = op["N"] + 8
        cbox, pbox = Boxed(op["M"] * ldc), Boxed(max(sp, 1) * op["M"] * op["N"])
        boxes.append((cbox, pbox, ldc))
        Ms[i] = _member(lib, op, cbox, ldc, pbox, sp, scale, jumps)
    sum_in = torch.randn(sum_n, generator=torch.Generator().manual_seed(sum_n)).cuda() if sum_n else None
    sum_out = Boxed(1) if sum_n else None
    lib.check(lib.load().d3p_gemm_f32_group(lib.stream_ptr(), Ms, len(ops), sp if sp > 1 else 0, lib.ptr(sum_in), None if sum_out is None else C.c_void_p(sum_out.x.data_ptr()), sum_n))
    torch.cuda.synchronize()
    res = []
    for i, (op, scale, jumps) in enumerate(ops):
        cbox, pbox, ldc = boxes[i]
        assert cbox.borders_intact() and pbox.borders_intact()
        kw = {} if scale is None else dict(b_row_scale=scale)
        alone = run(lib, op, ldc=ldc, jumps=jumps, part_splits=sp if sp > 1 else 0, force_splits=sp if sp > 1 else 0, leave_split=1, **kw)
        assert alone["route"] == BF16 and alone["left"] == (sp if sp > 1 else 0) == Ms[i].report.splits_left
        if sp > 1:
            assert bool((cbox.x == CANARY).all())
            res.append((Ms[i].joined, pbox.x.clone(), alone["part"]))
        else:
            res.append((Ms[i].joined, cbox.x.view(op["M"], ldc).clone(), alone["Cfull"]))
        assert Ms[i].report.route == (GROUPED if Ms[i].joined else BF16)
    return res, ops, (sum_in, sum_out)


@pytest.mark.parametrize("name", ["one", "two", "six", "mod", "odd"])
def test_grouped_launch_runs_the_members_tiles(lib, name):
    res, ops, _ = _run_group(lib, name)
    for joined, got, want in res:
        assert joined == 1 and torch.equal(got, want)
    op = ops[-1][0]      # the numbers themselves, once per group
    r = run(lib, op, jumps=ops[-1][2], ldc=op["N"] + 8, **({} if ops[-1][1] is None else dict(b_row_scale=ops[-1][1])))
    pre = op if ops[-1][1] is None else dict(op, b=op["b"] * ops[-1][1].view(-1, 1))
    assert_product(r["C"], *reference(pre), BF16, op["K"])


def test_a_seventh_member_and_one_of_another_form_are_launched_alone(lib):
    res, _, _ = _run_group(lib, "seven")
    assert [j for j, _, _ in res] == [1] * 6 + [0]
    for _, got, want in res:
        assert torch.equal(got, want)
    other = (make_operands("nn", 129, 68, 200, 55, a_last_one=True), None, None)      # a k-fast A among m-fast ones
    res, _, _ = _run_group(lib, "two", extra=other)
    assert [j for j, _, _ in res] == [1, 0, 1]
    for _, got, want in res:
        assert torch.equal(got, want)


@pytest.mark.parametrize("n", [1, 511, 512, 513, 4096])
def test_grouped_launch_sums_beside_its_products(lib, n):
    plain, _, _ = _run_group(lib, "two")
    res, _, (sum_in, sum_out) = _run_group(lib, "two", sum_n=n)
    assert sum_out.borders_intact()
    x = sum_in.double().cpu()
    assert abs(float(sum_out.x[0]) - float(x.sum())) <= n * 2.0 ** -24 * float(x.abs().sum())
    for (j0, a, _), (j1, b, _) in zip(plain, res):      # the extra workgroup shifts every slot by one: the members' outputs must not move
        assert j0 == j1 == 1 and torch.equal(a, b)


# ---- hostile operands beyond the plain form ------------------------------------------------------------------------------
@pytest.mark.parametrize("form,sp", [("nt", 0), ("tn", 0), ("tt", 0), ("nn", 3), ("tn", 3)])
def test_hostile_operands_in_every_form_and_split(lib, form, sp):
    M, N, K = 129, 68, 200
    A, Bm = R.hostile(M, N, K)
    op = make_operands(form, M, N, K, 1, A=A, Bm=Bm)
    r = run(lib, op, part_splits=sp, force_splits=sp)
    assert (r["route"], r["splits"]) == (BF16, max(sp, 1))
    ref, scale = reference(op)
    err = ((r["C"].double().cpu() - ref).abs() / scale).max()
    assert float(err) <= 3e-6, float(err)
    assert bool(torch.isfinite(r["C"]).all())


# ---- non-finite padding ----------------------------------------------------------------------------------------------------------
def _pad_cases(big):
    M, N = (129, 68) if big else (62, 65)
    return [("nn", M, N, 50), ("nt", M, N, 50), ("tn", M + 1, N, 52), ("tt", M, N, 50), ("tn", M, N, 33)]     # (M % 4 != 0 everywhere)


def _pad_strides(form, m_real, N, K):
    """Row strides with padding behind every fast extent that an eight-wave kernel may over-read (at least to roundup4)."""
    lda = (R.rup4(K) if K % 4 else K + 4) if form[0] == "n" else (R.rup4(m_real) if m_real % 4 else m_real + 4)
    return dict(lda=lda, ldb=R.rup4(N) if form[1] == "n" else R.rup4(K))


@pytest.mark.parametrize("fill", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("a_last_one", [False, True])
@pytest.mark.parametrize("big", [True, False])
def test_non_finite_padding_stays_out(lib, big, a_last_one, fill):
    """What lies between K and the row stride of a k-fast operand, and between M and the row stride of an m-fast A, is over-read by
    the eight-wave kernels (whole 16-byte loads) and must be masked whatever it holds: the product equals the same call with zeros
    there, and is finite."""
    for form, M, N, K in _pad_cases(big):
        M = M + 1 if a_last_one else M
        st = _pad_strides(form, M - 1 if a_last_one else M, N, K)
        bad = make_operands(form, M, N, K, 31, a_last_one=a_last_one, pad=fill, **st)
        zero = make_operands(form, M, N, K, 31, a_last_one=a_last_one, pad=0.0, **st)
        rb, rz = run(lib, bad), run(lib, zero)
        assert rb["route"] == rz["route"] and (rb["route"] == BF16) == big, (form, M, N, K)
        assert bool(torch.isfinite(rb["C"]).all()), (form, M, N, K)
        assert torch.equal(rb["C"], rz["C"]), (form, M, N, K)
        assert_product(rb["C"], *reference(zero), rb["route"], K)


@pytest.mark.parametrize("big", [True, False])
def test_a_nan_inside_the_matrix_reaches_its_row_or_column(lib, big):
    M, N, K = (129, 68, 50) if big else (63, 65, 17)
    for form in R.FORMS:
        op = make_operands(form, M, N, K, 41, big=big)
        a = op["a"]
        (a[3, 10:11] if form[0] == "n" else a[10, 3:4]).fill_(float("nan"))
        r = run(lib, op)
        bad = torch.isnan(r["C"])
        assert bool(bad[3].all()) and int(bad.sum()) == N, form
        op = make_operands(form, M, N, K, 41, big=big)
        b = op["b"]
        (b[10, 5:6] if form[1] == "n" else b[5, 10:11]).fill_(float("nan"))
        r = run(lib, op)
        bad = torch.isnan(r["C"])
        assert bool(bad[:, 5].all()) and int(bad.sum()) == M, form


# ---- the eight-wave fp32 kernel under its developer switch -------------------------------------------------------------------
def w8_child():
    """Runs in a fresh process with D3P_GEMM_FP32_MFMA=1 (the switch is read once per process): k_gemm_f32_w8 at the product tolerance."""
    import d3p_amd._lib as L
    L.load()
    L.require_device()
    for M, N, K in [(129, 68, 31), (260, 100, 200), R.DEEP]:
        for form in R.FORMS:
            op = make_operands(form, M, N, K, M + K)
            bias = torch.randn(N, generator=torch.Generator().manual_seed(K)).cuda()
            r = run(L, op, bias=bias, alpha=0.5)
            assert (r["route"], r["splits"]) == (W8, 1), (r["route"], form, M, N, K)
            assert_product(r["C"], *reference(op, bias, 0.5), W8, K)
    op = make_operands("tn", 130, 68, 100, 3, a_last_one=True)
    r = run(L, op)
    assert r["route"] == W8
    assert_product(r["C"], *reference(op), W8, 100)
    op = make_operands("nn", 129, 64, 200, 4)      # 2 tiles, `part` alone: K / 64 = 3 slabs allowed, K ranges of 96: 96 / 96 / 8
    red, left = run(L, op, part_splits=16), run(L, op, part_splits=16, leave_split=1)
    assert red["route"] == left["route"] == W8 and red["splits"] == left["left"] == 3, (red["splits"], left["left"])
    assert torch.equal(tile_sum(left["part"], 3, 129, 64), red["C"])
    assert_product(red["C"], *reference(op), W8, 200)
    for form, M, N, K in _pad_cases(True):
        st = _pad_strides(form, M, N, K)
        rb, rz = run(L, make_operands(form, M, N, K, 31, pad=float("nan"), **st)), run(L, make_operands(form, M, N, K, 31, pad=0.0, **st))
        assert rb["route"] == W8 and torch.equal(rb["C"], rz["C"]) and bool(torch.isfinite(rb["C"]).all()), form
    print("w8 child ok")


def test_fp32_eight_wave_kernel_under_its_switch(lib):
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_vae_gemm as T; T.w8_child()" % (os.path.dirname(here), here)
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, D3P_GEMM_FP32_MFMA="1"), timeout=300)


def test_zz_epilogue_ratios_are_reported(lib):
    """(last in the file) the worst device error / bound per epilogue output over the cases above."""
    for k in sorted(RATIOS):
        print(f"ratio {k}: {RATIOS[k]:.3f}")
    assert all(v <= 1.0 for v in RATIOS.values())
