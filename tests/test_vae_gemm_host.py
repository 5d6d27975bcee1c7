"""Host checks of tests/vae_gemm_ref.py (no GPU): the float64 restatement against torch.matmul on dense copies, the epilogue
formulas against autograd on the terms they claim to differentiate, and the case lists against the axes they must cover."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_gemm_ref as R  # noqa: E402


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("a_last_one", [False, True])
def test_strided_product_equals_matmul_on_dense_copies(form, a_last_one):
    M, N, K = 7, 5, 6
    g = torch.Generator().manual_seed(1)
    m_real = M - 1 if a_last_one else M
    A, Bm = torch.randn(m_real, K, generator=g), torch.randn(K, N, generator=g)
    a_sm, a_sk, b_sk, b_sn, sa, sb = R.form_strides(form, m_real, K, N, lda=(K if form[0] == "n" else m_real) + 3, ldb=(N if form[1] == "n" else K) + 2)
    a_st, b_st = torch.randn(sa, generator=g), torch.randn(sb, generator=g)
    a_st[:, :(K if form[0] == "n" else m_real)] = A if form[0] == "n" else A.t()
    b_st[:, :(N if form[1] == "n" else K)] = Bm if form[1] == "n" else Bm.t()
    Ad, Bd = R.operands(a_st, a_sm, a_sk, b_st, b_sk, b_sn, M, N, K, a_last_one)
    dense = torch.cat([A, torch.ones(1, K)]) if a_last_one else A
    assert torch.equal(Ad, dense.double()) and torch.equal(Bd, Bm.double())
    bias, C0 = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    o, scale = R.product(Ad, Bd, bias, 0.5, C0)
    want = 0.5 * torch.matmul(dense.double(), Bm.double()) + bias.double() + C0.double()
    assert torch.allclose(o, want, rtol=0, atol=1e-14)
    assert torch.equal(scale, torch.matmul(dense.double().abs(), Bm.double().abs()))


def test_displaced_segments_are_gathered():
    K, N, n_seg, k_seg = 5, 6, 4, 3
    jumps = dict(n_seg=n_seg, k_seg=k_seg, b_njump=40, b_kjump=100, bias_njump=7, c_njump=2)
    flat = torch.arange(400.0)
    _, B = R.operands(torch.zeros(2 * K), K, 1, flat, N, 1, 2, N, K, False, jumps)
    for k in range(K):
        for n in range(N):
            assert float(B[k, n]) == k * N + n + (40 if n >= n_seg else 0) + (100 if k >= k_seg else 0)
    assert R.gather_bias(flat, N, jumps).tolist() == [0, 1, 2, 3, 11, 12]
    assert R.c_columns(N, jumps).tolist() == [0, 1, 2, 3, 6, 7]
    assert R.c_columns(N).tolist() == list(range(N))


def test_fma_round_rounds_once():
    s, b = torch.tensor([1.0 + 2.0 ** -23]), torch.tensor([-(2.0 ** -25)])
    # 0.75 s + b = 0.75 + 1.5 * 2^-24 - 0.5 * 2^-24 = 0.75 + 2^-24 exactly; rounding the product first (a tie, to even) gives 0.75 + 2^-23
    assert float(R.fma_round(0.75, s, b)[0]) == 0.75 + 2.0 ** -24
    assert float((torch.tensor(0.75) * s + b)[0]) == 0.75 + 2.0 ** -23


def test_epilogue_1_is_softplus_and_its_derivative():
    o = torch.linspace(-30, 30, 121, dtype=torch.float64, requires_grad=True)
    sp, sg = R.epi1(o)
    assert torch.allclose(sp, torch.logaddexp(torch.zeros_like(o), o), rtol=1e-13, atol=0)      # log(1 + e^o)
    (grad,) = torch.autograd.grad(torch.logaddexp(torch.zeros_like(o), o).sum(), o)      # (of the definition: |o| has no derivative at 0)
    assert torch.allclose(sg, grad, rtol=1e-13, atol=1e-300)
    inf = torch.tensor([float("inf"), 0.0, -0.0], dtype=torch.float64)
    sp, sg = R.epi1(inf)
    assert sp.tolist() == [float("inf"), R.math.log(2.0), R.math.log(2.0)] and sg.tolist() == [1.0, 0.5, 0.5]


def test_epilogue_2_is_the_chain_rule_through_softplus():
    g = torch.Generator().manual_seed(2)
    pre = torch.randn(4, 5, generator=g, dtype=torch.float64, requires_grad=True)
    up = torch.randn(4, 5, generator=g, dtype=torch.float64)          # the gradient arriving at h = softplus(pre)
    h, sig = R.epi1(pre)
    (grad,) = torch.autograd.grad((h * up).sum(), pre)
    assert torch.allclose(R.epi2(up, sig.detach()), grad, rtol=1e-13, atol=0)


def test_epilogue_3_is_the_gradient_through_the_reparametrised_latent():
    """z = loc + exp(u) eps; the terms of the loss that see z beside the decoder (gradient o): sc z^2 / 2 (the prior) and - sc u (the
    guide's entropy).  d / d loc = o + sc z = dz, d / d u = dz sd eps - sc = du."""
    g = torch.Generator().manual_seed(3)
    M, Z, sc = 4, 3, 0.75
    loc = torch.randn(M, Z, generator=g, dtype=torch.float64, requires_grad=True)
    u = torch.randn(M, Z, generator=g, dtype=torch.float64, requires_grad=True)
    eps, o = torch.randn(M, Z, generator=g, dtype=torch.float64), torch.randn(M, Z, generator=g, dtype=torch.float64)
    sd = torch.exp(u)
    z = loc + sd * eps
    loss = (o * z).sum() + sc * 0.5 * (z * z).sum() - sc * u.sum()
    gl, gu = torch.autograd.grad(loss, (loc, u))
    dz, du = R.epi3(o, z.detach(), sd.detach(), eps, sc)
    assert torch.allclose(dz, gl, rtol=1e-13, atol=1e-15) and torch.allclose(du, gu, rtol=1e-13, atol=1e-15)


def test_epilogue_4_is_the_bernoulli_gradient_and_its_row_sums():
    g = torch.Generator().manual_seed(4)
    M, N, sc = 3, 70, 1.25
    o = (3 * torch.randn(M, N, generator=g, dtype=torch.float64)).requires_grad_()
    x = torch.rand(M, N, generator=g, dtype=torch.float64)
    ll = (x * o - torch.nn.functional.softplus(o))                 # log Bernoulli(x | logits o)
    assert torch.allclose(ll, x * torch.nn.functional.logsigmoid(o) + (1 - x) * torch.nn.functional.logsigmoid(-o), rtol=1e-12, atol=1e-14)
    (grad,) = torch.autograd.grad(-sc * ll.sum(), o)
    c, gll, gxx = R.epi4(o.detach(), x, sc)
    assert torch.allclose(c, grad, rtol=1e-13, atol=1e-15)
    assert gll.shape == gxx.shape == (3, M)                          # ceil(70 / 32) groups
    assert torch.allclose(gll.sum(0), ll.detach().sum(1), rtol=1e-13) and torch.allclose(gxx.sum(0), (x * x).sum(1), rtol=1e-13)
    assert torch.allclose(gll[2], ll.detach()[:, 64:].sum(1), rtol=1e-13)


def test_epilogue_bounds_are_float32_sized():
    g = torch.Generator().manual_seed(5)
    o = 5 * torch.randn(50, 40, generator=g)
    for b in R.epi_bounds("epi1", o):
        assert 2.0 ** -26 < b < 4 * 8 * 2.0 ** -24
    x = torch.rand(50, 40, generator=g)
    for b in R.epi_bounds("epi4", o, x, 1.25):
        assert 0 < b < 4 * 40 * 2.0 ** -24


def test_split_arithmetic():
    assert R.split_count_ok(3, 200) == (True, 96) and R.slabs(200, 96) == [96, 96, 8]
    assert R.split_count_ok(2, 100) == (True, 64) and R.slabs(100, 64) == [64, 36]
    assert not R.split_count_ok(5, 200)[0] and not R.split_count_ok(2, 64)[0] and not R.split_count_ok(17, 4096)[0]
    assert R.f32_split_count(65, 5, 200) == 3 and R.f32_split_count(1, 1, 500) == 7 and R.f32_split_count(64, 64, 70) == 1


def test_case_lists_cover_every_axis():
    big = R.BIG_SHAPES + [c[:3] for c in R.BIG_SPLITS]
    assert set(R.BIG_M) <= {M for M, N, K in big} and set(R.BIG_N) <= {N for M, N, K in big} and set(R.BIG_K) <= {K for M, N, K in big}
    assert R.DEEP in R.BIG_SHAPES and R.DEEP[0] == 51 and R.DEEP[2] == 2048
    for M, N, K in big:      # every one takes the eight-wave kernels in every form: M > 96 or deep, N % 4 == 0
        assert (M > 96 or (M > 32 and K >= 2048)) and N % 4 == 0
    for M, N, K, sp in R.BIG_SPLITS:
        assert R.split_count_ok(sp, K)[0]
    assert any(R.slabs(K, R.split_count_ok(sp, K)[1])[-1] < R.GKB for M, N, K, sp in R.BIG_SPLITS)      # a last slab shorter than a slice
    f32 = R.F32_SHAPES + R.F32_SPLITS
    assert set(R.F32_MN) <= {M for M, N, K in f32} and set(R.F32_MN) <= {N for M, N, K in f32} and set(R.F32_K) <= {K for M, N, K in R.F32_SHAPES}
    for M, N, K in f32:
        assert M <= 130 and N <= 130
    for M, N, K in R.F32_SPLITS:
        assert K >= 128 and R.f32_split_count(M, N, K) > 1
    assert {R.f32_route(f, M, N, K) for f in R.FORMS for M, N, K in R.F32_SHAPES} == {0, 1, 2, 3}
    tb, tf = R.tile_counts()
    assert {t % 8 for t in tb} == set(range(8)) and {t % 8 for t in tf} == set(range(8))
    assert min(tb) < 8 and min(tf) < 8 and max(tb) > 8 and max(tf) > 8


def test_group_lists_cover_every_workgroup_count():
    assert {c % 8 for c in R.group_counts()} == set(range(8))
    assert {len(g["members"]) for g in R.GROUPS.values()} >= {1, 2, 6, 7}
    for g in R.GROUPS.values():
        assert R.split_count_ok(g["splits"], g["K"])[0] and len(g["members"]) <= R.GROUP_MAX + 1
        for M, N in g["members"]:
            assert M > 96 and N % 4 == 0


def test_hostile_operands_are_what_they_claim():
    A, Bm = R.hostile(8, 4, 14)
    assert float(A[0, 0]) == float(torch.nextafter(torch.tensor(2.0), torch.tensor(0.0)))
    assert torch.equal(A[:, 1::2], -A[:, 0::2] * (1.0 + 2.0 ** -12)) and torch.equal(Bm[1::2], Bm[0::2])
    assert float(A.abs().max() / A.abs().min()) > 2.0 ** 12
