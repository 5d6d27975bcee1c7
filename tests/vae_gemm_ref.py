"""Float64 restatement of the VAE's product dispatcher (d3p_amd/csrc/d3p_gemm.hip: gemm(), GemmArgs) for tests/test_gpu_vae_gemm.py
and tests/test_vae_gemm_host.py: strided products with bias, alpha and accumulate, the virtual row of ones, the displaced
segments, the four epilogues from their definitions, a float32 restatement of the epilogues that calibrates their tolerance, and
the case lists.  No device code; everything runs on the CPU in torch.

Tolerances (the project's figures, tests/test_gpu_vae.py): fp32 kernels 2e-5 of max sum_k |a||b|; bf16x3 kernel 3e-6 of each
element's sum_k |a||b| at K <= 1024, 2e-5 of the max beyond.  Epilogues: four times the worst error of the float32 torch
restatement against float64 on the same inputs (the rule of tests/glm_ref.py), errors taken relative to max(|value|, natural scale)."""
import math

import torch

F64 = torch.float64
TOL_F32, TOL_BF16 = 2e-5, 3e-6
GKB, GTM, GT, GK = 32, 128, 64, 16      # K slice and tile rows of the eight-wave kernels; tile edge and K slice of the 64 x 64 kernel
GROUP_MAX, WPART_SPLITS = 6, 16


# ---- strided operands ------------------------------------------------------------------------------------------------------------
def strided(flat, n0, n1, s0, s1, off0=None, off1=None):
    """float64 [n0, n1] with element (i, j) = flat[i s0 + j s1 + off0[i] + off1[j]]."""
    i = torch.arange(n0).view(-1, 1) * s0 + (0 if off0 is None else off0.view(-1, 1))
    j = torch.arange(n1).view(1, -1) * s1 + (0 if off1 is None else off1.view(1, -1))
    return flat.detach().cpu().reshape(-1)[(i + j).reshape(-1)].reshape(n0, n1).to(F64)


def seg_offsets(n, seg, jump):
    """Offsets of the displaced segments: indices >= seg lie `jump` elements further."""
    return (torch.arange(n) >= seg).long() * jump


def operands(a_flat, a_sm, a_sk, b_flat, b_sk, b_sn, M, N, K, a_last_one=False, jumps=None):
    """The dense float64 op(A) [M, K] and op(B) [K, N]: the row of ones appended, the displaced segments of B gathered."""
    m_real = M - 1 if a_last_one else M
    A = strided(a_flat, m_real, K, a_sm, a_sk)
    if a_last_one:
        A = torch.cat([A, torch.ones(1, K, dtype=F64)])
    if jumps is None:
        B = strided(b_flat, K, N, b_sk, b_sn)
    else:
        B = strided(b_flat, K, N, b_sk, b_sn, seg_offsets(K, jumps["k_seg"], jumps["b_kjump"]), seg_offsets(N, jumps["n_seg"], jumps["b_njump"]))
    return A, B


def product(A, B, bias=None, alpha=1.0, C0=None):
    """o = alpha A B + bias (+ C0) in float64, and sum_k |a||b| per element (the products' error scale)."""
    o = float(alpha) * (A @ B)
    if bias is not None:
        o = o + bias.detach().cpu().to(F64).view(1, -1)
    if C0 is not None:
        o = o + C0.detach().cpu().to(F64)
    return o, A.abs() @ B.abs()


def gather_bias(bias_flat, N, jumps=None):
    idx = torch.arange(N) + (0 if jumps is None else seg_offsets(N, jumps["n_seg"], jumps["bias_njump"]))
    return bias_flat.detach().cpu().reshape(-1)[idx]


def c_columns(N, jumps=None):
    """Where column n of the product lies in a row of C."""
    return torch.arange(N) + (0 if jumps is None else seg_offsets(N, jumps["n_seg"], jumps["c_njump"]))


def fma_round(alpha, s, bias):
    """float32 fma(alpha, s, bias) of float32 inputs: exact in float64 (24 + 24 bit product, one aligned add of numbers whose
    exponents differ by far less than 2^29 here), rounded once."""
    return (float(alpha) * s.to(F64) + bias.to(F64)).to(torch.float32)


# ---- epilogues, from their definitions (GemmArgs::epi); dtype = float64 for the reference, float32 for the calibration -------
def softplus(o):
    return torch.clamp(o, min=0) + torch.log1p(torch.exp(-o.abs()))


def epi1(o, dtype=F64):
    """C = softplus(o), C2 = sigmoid(o) = softplus'(o)."""
    o = o.to(dtype)
    return softplus(o), torch.sigmoid(o)


def epi2(o, c2, dtype=F64):
    """C = o * C2."""
    return o.to(dtype) * c2.to(dtype)


def epi3(o, z, sd, eps, sc, dtype=F64):
    """The backward pass through the reparametrised latent: dz = o + sc z, du = dz sd eps - sc."""
    o, z, sd, eps = (t.to(dtype) for t in (o, z, sd, eps))
    sc = torch.tensor(sc, dtype=torch.float32).to(dtype)
    dz = o + sc * z
    return dz, dz * sd * eps - sc


def col_groups(t, width=32):
    """[M, N] -> [ceil(N / 32), M]: sums over groups of 32 columns."""
    M, N = t.shape
    G = (N + width - 1) // width
    pad = torch.zeros(M, G * width, dtype=t.dtype)
    pad[:, :N] = t
    return pad.view(M, G, width).sum(2).t().contiguous()


def epi4(o, x, sc, dtype=F64):
    """The decoder's output layer: C = sc (sigmoid(o) - x); per row and 32 columns the sums of x o - softplus(o) and of x^2."""
    o, x = o.to(dtype), x.to(dtype)
    sc = torch.tensor(sc, dtype=torch.float32).to(dtype)
    return sc * (torch.sigmoid(o) - x), col_groups(x * o - softplus(o)), col_groups(x * x)


def epi_scales(name, o, *ops):
    """The natural scale of every output of an epilogue (float64): errors are relative to max(|value|, scale)."""
    o = o.to(F64)
    ops = [t.to(F64) if torch.is_tensor(t) else t for t in ops]
    if name == "epi1":
        return [o.abs() + math.log(2.0), torch.ones_like(o)]
    if name == "epi2":
        return [(o * ops[0]).abs()]
    if name == "epi3":
        z, sd, eps, sc = ops
        dz = o + sc * z
        return [o.abs() + (sc * z).abs(), (dz * sd * eps).abs() + abs(sc)]
    if name == "epi4":
        x, sc = ops
        return [abs(sc) * (1.0 + x.abs()), col_groups((x * o).abs() + o.abs() + math.log(2.0)), col_groups(x * x)]
    raise KeyError(name)


_EPI = {"epi1": epi1, "epi2": epi2, "epi3": epi3, "epi4": epi4}


def rel_errors(got, ref, scales):
    """Worst error of every output relative to max(|ref|, scale), over the finite reference values; a non-finite reference value must
    be met exactly."""
    out = []
    for g, r, s in zip(got, ref, scales):
        g, r = g.to(F64), r.to(F64)
        fin = torch.isfinite(r)
        assert torch.equal(g[~fin], r[~fin]), "non-finite values differ"
        den = torch.maximum(r.abs(), s.to(F64)).clamp_min(1e-300)
        out.append(float(((g - r).abs() / den)[fin].max()) if bool(fin.any()) else 0.0)
    return out


def epi_outputs(name, o, *ops, dtype=F64):
    res = _EPI[name](o, *ops, dtype=dtype)
    return list(res) if isinstance(res, tuple) else [res]


def epi_bounds(name, o, *ops):
    """Per output of the epilogue: 4 x the worst relative error of the float32 torch restatement against float64 on these inputs."""
    ref = epi_outputs(name, o, *ops)
    f32 = epi_outputs(name, o, *ops, dtype=torch.float32)
    return [4.0 * e for e in rel_errors(f32, ref, epi_scales(name, o, *ops))]


# ---- the dispatcher's split arithmetic, restated ------------------------------------------------------------------------------
def split_count_ok(sp, K):
    """Can the dispatcher's own split choice return sp for K (bf16 kernel)?  Returns (ok, k_per)."""
    if sp < 1 or sp > WPART_SPLITS:
        return False, 0
    kp = -(-(-(-K // sp)) // GKB) * GKB
    return (-(-K // kp) == sp and kp >= 2 * GKB), kp


def slabs(K, k_per):
    return [min(k_per, K - z * k_per) for z in range(-(-K // k_per))]


def tiles_big(M, N):
    return -(-M // GTM) * -(-N // GT)


def tiles_f32(M, N):
    return -(-M // GT) * -(-N // GT)


def f32_split_count(M, N, K):
    """Splits the 64 x 64 kernel takes when `part` is given (gemm(): 1024 workgroups wanted, K ranges of 64 or more, 16 at most)."""
    t = tiles_f32(M, N)
    if not (t < 512 and K >= 8 * GK):
        return 1
    sp = min(-(-1024 // t), K // (4 * GK), 16)
    kp = -(-(-(-K // max(sp, 1))) // GK) * GK
    return -(-K // kp)


FORMS = ("nn", "nt", "tn", "tt")


def form_strides(form, M, K, N, lda=None, ldb=None):
    """(a_sm, a_sk, b_sk, b_sn, A storage shape, B storage shape) of an operand form; lda / ldb = padded row strides."""
    if form[0] == "n":
        lda = K if lda is None else lda
        a = (lda, 1, (M, lda))
    else:
        lda = M if lda is None else lda
        a = (1, lda, (K, lda))
    if form[1] == "n":
        ldb = N if ldb is None else ldb
        b = (ldb, 1, (K, ldb))
    else:
        ldb = K if ldb is None else ldb
        b = (1, ldb, (N, ldb))
    return a[0], a[1], b[0], b[1], a[2], b[2]


def rup4(v):
    return (v + 3) & ~3


def big_strides(form, M, K, N):
    """Row strides with which every form of (M, N, K) is 16-byte loadable by the eight-wave kernels: roundup4 of the fast extent."""
    return form_strides(form, M, K, N, lda=rup4(K) if form[0] == "n" else rup4(M), ldb=rup4(N) if form[1] == "n" else rup4(K))


def f32_route(form, M, N, K):
    """The 64 x 64 kernel's VA / VB bits for dense operands of this form (gemm(): K % 4 == 0 and the other stride % 4 == 0)."""
    other_a = K if form[0] == "n" else M
    other_b = N if form[1] == "n" else K
    return (1 if K % 4 == 0 and other_a % 4 == 0 else 0) | (2 if K % 4 == 0 and other_b % 4 == 0 else 0)


# ---- case lists ----------------------------------------------------------------------------------------------------------------
# axes the lists must cover (tests/test_vae_gemm_host.py checks that they do)
BIG_M, BIG_N, BIG_K = (97, 128, 129, 260), (4, 64, 68, 100, 132), (1, 3, 31, 32, 33, 50, 64, 96, 100, 200)
F32_MN, F32_K = (1, 5, 63, 64, 65, 130), (1, 3, 15, 16, 17, 70)
DEEP = (51, 68, 2048)   # the short, very deep product: M > 32 with K >= 2048 takes the eight-wave kernels too

# eight-wave kernels (bf16x3; k_gemm_f32_w8 under the switch): (M, N, K), every one with N % 4 == 0 (an n-fast B needs it)
BIG_SHAPES = [(97, 4, 1), (128, 64, 3), (129, 68, 31), (260, 100, 32), (97, 132, 33), (129, 100, 50), (260, 64, 64), (128, 132, 96),
              (260, 132, 100), (129, 64, 200), (260, 68, 200), DEEP]
# split cases of the eight-wave kernels: (M, N, K, force_splits); K = 200 in three slabs is 96 / 96 / 8, K = 100 in two 64 / 36
BIG_SPLITS = [(129, 64, 200, 3), (260, 132, 200, 3), (97, 68, 100, 2), (260, 100, 96, 2), (128, 132, 200, 2), (51, 64, 2048, 5),
              (51, 64, 2048, 7), (51, 4, 2048, 16)]
# 64 x 64 kernel
F32_SHAPES = [(1, 1, 1), (5, 63, 3), (63, 5, 15), (64, 64, 16), (65, 130, 17), (130, 65, 70), (65, 130, 16), (130, 130, 15), (64, 1, 70), (1, 64, 16), (65, 65, 3)]
# its split cases (`part` alone, K >= 128): K = 200 -> 80 / 80 / 40, 330 -> 4 x 80 + 10, 500 -> 6 x 80 + 20
F32_SPLITS = [(64, 64, 128), (65, 5, 200), (5, 63, 330), (1, 1, 500), (130, 130, 200), (63, 130, 128), (65, 65, 128)]


def tile_counts():
    """T = tiles x splits of every launch in the lists, per kernel."""
    big = [tiles_big(M, N) for M, N, K in BIG_SHAPES] + [tiles_big(M, N) * sp for M, N, K, sp in BIG_SPLITS]
    f32 = [tiles_f32(M, N) for M, N, K in F32_SHAPES] + [tiles_f32(M, N) * f32_split_count(M, N, K) for M, N, K in F32_SPLITS]
    return big, f32


# grouped launches: members (M - 1 rows of A in memory + the row of ones, N, ldc), one K and force_splits per group; the workgroup
# counts cnt = tiles x splits of the members cover cnt mod 8 = 0 .. 7
GROUPS = {
    "one": dict(K=200, splits=3, members=[(129, 64)]),                                        # cnt 6
    "two": dict(K=200, splits=1, members=[(97, 4), (260, 68)]),                               # cnt 1, 6
    "six": dict(K=320, splits=5, members=[(97, 64), (129, 132), (260, 100), (128, 4), (260, 132), (385, 68)]),   # cnt 5, 30, 30, 5, 45, 40
    "mod": dict(K=200, splits=1, members=[(129, 100), (260, 132), (97, 132), (385, 100), (500, 100), (129, 64)]),   # cnt 4, 9, 3, 8, 8, 2
    "seven": dict(K=100, splits=2, members=[(97, 4)] * 6 + [(129, 68)]),                      # cnt 2 x 6, the seventh alone
    "odd": dict(K=448, splits=7, members=[(97, 64), (128, 64)]),                              # cnt 7, 7
}


def group_counts():
    return [tiles_big(M, N) * g["splits"] for g in GROUPS.values() for M, N in g["members"]]


def hostile(M, N, K, seed=77):
    """The operands of test_split_product_is_fp32_accurate_on_hostile_operands: exponents spanning 2^+-20, every significand bit set,
    cancelling pairs."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-20, 21, (M, K), generator=g).float())
    Bm = torch.randn(K, N, generator=g) * torch.exp2(torch.randint(-20, 21, (K, N), generator=g).float())
    A[:, ::7] = torch.nextafter(torch.tensor(2.0), torch.tensor(0.0))
    Bm[::5, :] = torch.nextafter(torch.tensor(-1.0), torch.tensor(0.0))
    A[:, 1::2] = -A[:, 0::2] * (1.0 + 2.0 ** -12)
    Bm[1::2, :] = Bm[0::2, :]
    return A, Bm
