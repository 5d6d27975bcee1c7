// The strided matrix products of the VAE's DP-VI step (d3p_vae.hip) on the matrix cores: the kernels, the one routing rule
// (gemm_route), the dispatcher gemm(), the grouped launch, and the C entries that make the layer testable on its own.
#include <type_traits>
#include "d3p_gemm.h"

namespace d3p {

// ------------------------------------------------------------------------------------------------------------------
// C[M x N] = alpha * sum_k A(m, k) B(k, n) (+ bias[n]) (+ C),  A(m, k) = A[m * a_sm + k * a_sk], B(k, n) = B[k * b_sk + n * b_sn]
// (element strides cover NN / NT / TN), C row-major with leading dimension ldc.
// Workgroup = 4 wavefronts (2 x 2), tile 64 x 64, K in slices of 16 staged through LDS; every wavefront owns a 32 x 32
// accumulator = 16 VGPRs of v_mfma_f32_32x32x2_f32 (lane l: A row / B column l % 32, k = l / 32; D[i][j] with
// j = l % 32, i = 8 (v / 4) + 4 (l / 32) + v % 4).
// ------------------------------------------------------------------------------------------------------------------
typedef float float16v __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(256) k_exact16_flag(const float* __restrict__ x, size_t n4, uint32_t* __restrict__ flag, uint32_t nonce)
{
    exact16_pass(x, n4, flag, nonce, blockIdx.x, gridDim.x);
}

void exact16_flag_launch(hipStream_t s, const float* x, size_t n4, uint32_t* flag, uint32_t nonce)
{
    hipLaunchKernelGGL(k_exact16_flag, dim3(exact16_blocks(n4)), dim3(256), 0, s, x, n4, flag, nonce);
}

// o = alpha * acc + bias (+ C); then the epilogue
__device__ __forceinline__ void gemm_store(const GemmArgs& g, int row, int col, float acc, float bv)
{
    const size_t e = (size_t)row * g.ldc + col + (col >= g.n_seg ? g.c_njump : 0ll);
    float o = __fmaf_rn(g.alpha, acc, bv);
    if (g.accumulate) o += g.C[e];
    if (g.epi == 1) {  // one exponential: en = exp(-|o|); sigmoid = 1 / (1 + en) or en / (1 + en); softplus = max(o, 0) + log(1 + en)
        const float en = __expf(-fabsf(o)), r = __builtin_amdgcn_rcpf(1.0f + en);
        g.C2[e] = o >= 0.0f ? r : en * r;
        o = fmaxf(o, 0.0f) + __logf(1.0f + en);
    } else if (g.epi == 2) {
        o *= g.C2[e];
    } else if (g.epi == 3) {
        o = __fmaf_rn(g.ex_sc, g.ex_zu[e], o);
        g.C[e + g.ex_Z] = o * g.ex_zu[e + g.ex_Z] * g.ex_eps[(size_t)row * g.ex_Z + col] - g.ex_sc;
    }
    g.C[e] = o;
}

// XCD-aware tile order.  The chip's 8 XCDs have an L2 each and workgroups are dealt to them round-robin by linear id, so with the
// natural blockIdx -> tile mapping the tiles that SHARE operand data (the N-tiles of one M row block; the tiles of one split-K
// slab) land on 8 different L2s and every XCD streams (nearly) the whole of A and B from memory: 134 MB for the 14 MB h1 product.
// Here workgroup L (XCD L % 8, the j = L / 8-th workgroup of that XCD) takes tile R = start(XCD) + j of the reuse order
// n-fastest, then m, then the K slab: every XCD works through ONE contiguous run of that order, so an A row block is fetched into
// one L2 once and hit by the other N-tiles.  (Only locality depends on the round-robin assumption; the mapping is a bijection.)
__device__ __forceinline__ void xcd_tile(int& bx, int& by, int& bz)
{
    const unsigned gx = gridDim.x, gy = gridDim.y, T = gx * gy * gridDim.z;
    const unsigned L = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const unsigned c = L & 7u, j = L >> 3, base = T >> 3, r = T & 7u;
    const unsigned R = c * base + (c < r ? c : r) + j;
    bx = (int)(R % gx);
    by = (int)((R / gx) % gy);
    bz = (int)(R / (gx * gy));
}

// VA / VB: the operand is fetched with ONE 16-byte load per thread and slice along its unit-stride dimension (the host
// checks alignment and that the other stride and the extents are multiples of 4); otherwise 4 scalar loads with per-element
// guards.  The scalar form issues 8 loads per thread and slice, each behind 64-bit index arithmetic, and was the
// bottleneck of these GEMMs (adding one more dependent load per element cost +13 % on the whole step).
template <bool VA, bool VB>
__global__ void __launch_bounds__(256) k_gemm_f32(GemmArgs g)
{
    __shared__ __attribute__((aligned(16))) float As[D3P_GK][D3P_GT + 4];  // [k][m]
    __shared__ __attribute__((aligned(16))) float Bs[D3P_GK][D3P_GT + 4];  // [k][n]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int tx, ty, tz;
    xcd_tile(tx, ty, tz);
    const int m0 = ty * D3P_GT, n0 = tx * D3P_GT;
    const int kbeg = tz * g.k_per, kend = (kbeg + g.k_per < g.K) ? kbeg + g.k_per : g.K;
    float16v acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    // staging maps: the unit-stride dimension of each operand runs along consecutive threads
    const bool a_kfast = g.a_sk == 1, b_nfast = g.b_sn == 1;
    int am[4], ak[4], bk[4], bn[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = tid + 256 * r;  // 0 .. 1023
        if (a_kfast) { ak[r] = e & 15; am[r] = e >> 4; } else { am[r] = e & 63; ak[r] = e >> 6; }
        if (b_nfast) { bn[r] = e & 63; bk[r] = e >> 6; } else { bk[r] = e & 15; bn[r] = e >> 4; }
    }
    // vector maps: 4 consecutive elements of the fast dimension per thread
    const int vam = a_kfast ? (tid >> 2) : 4 * (tid & 15), vak = a_kfast ? 4 * (tid & 3) : (tid >> 4);
    const int vbn = b_nfast ? 4 * (tid & 15) : (tid >> 2), vbk = b_nfast ? (tid >> 4) : 4 * (tid & 3);
    const int m_real = g.a_last_one ? g.M - 1 : g.M;  // rows of A that exist in memory
    float ra[4], rb[4];
    auto fetch = [&](int k0) {  // global -> registers for the slice starting at k0
        if (VA) {
            const int gm = m0 + vam, gk = k0 + vak;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a_kfast) {  // 4 k of one row
                if (gm < m_real && gk < kend) v = *reinterpret_cast<const float4*>(g.A + (long long)gm * g.a_sm + gk);
                else if (gm < g.M && gk < kend) v = make_float4(1.f, 1.f, 1.f, 1.f);  // the virtual row of ones
            } else {        // 4 rows of one k
                if (gk < kend) {
                    if (gm + 3 < m_real) {
                        v = *reinterpret_cast<const float4*>(g.A + (long long)gk * g.a_sk + gm);
                    } else {
                        float t[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            t[i] = (gm + i < m_real) ? g.A[(long long)gk * g.a_sk + gm + i] : ((gm + i < g.M) ? 1.0f : 0.f);
                        v = make_float4(t[0], t[1], t[2], t[3]);
                    }
                }
            }
            ra[0] = v.x; ra[1] = v.y; ra[2] = v.z; ra[3] = v.w;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gm = m0 + am[r], gka = k0 + ak[r];
                float va = 0.f;
                if (gm < g.M && gka < kend)
                    va = (g.a_last_one && gm == g.M - 1) ? 1.0f : g.A[(long long)gm * g.a_sm + (long long)gka * g.a_sk];
                ra[r] = va;
            }
        }
        if (VB) {
            const int gn = n0 + vbn, gk = k0 + vbk;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b_nfast) {  // 4 n of one k
                if (gk < kend) {
                    if (gn + 3 < g.N) {
                        v = *reinterpret_cast<const float4*>(g.B + (long long)gk * g.b_sk + gn);
                    } else {
                        float t[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) t[i] = (gn + i < g.N) ? g.B[(long long)gk * g.b_sk + gn + i] : 0.f;
                        v = make_float4(t[0], t[1], t[2], t[3]);
                    }
                }
            } else {        // 4 k of one column
                if (gn < g.N && gk < kend) v = *reinterpret_cast<const float4*>(g.B + (long long)gn * g.b_sn + gk);
            }
            rb[0] = v.x; rb[1] = v.y; rb[2] = v.z; rb[3] = v.w;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gkb = k0 + bk[r], gn = n0 + bn[r];
                rb[r] = (gkb < kend && gn < g.N)
                            ? g.B[(long long)gkb * g.b_sk + (long long)gn * g.b_sn + (gn >= g.n_seg ? g.b_njump : 0ll) + (gkb >= g.k_seg ? g.b_kjump : 0ll)]
                            : 0.f;
            }
        }
    };
    auto stage = [&]() {  // registers -> LDS
        if (VA) {
            if (a_kfast) {
#pragma unroll
                for (int i = 0; i < 4; ++i) As[vak + i][vam] = ra[i];
            } else {
                *reinterpret_cast<float4*>(&As[vak][vam]) = make_float4(ra[0], ra[1], ra[2], ra[3]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) As[ak[r]][am[r]] = ra[r];
        }
        if (VB) {
            if (b_nfast) {
                *reinterpret_cast<float4*>(&Bs[vbk][vbn]) = make_float4(rb[0], rb[1], rb[2], rb[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) Bs[vbk + i][vbn] = rb[i];
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) Bs[bk[r]][bn[r]] = rb[r];
        }
    };
    if (kbeg < kend) fetch(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += D3P_GK) {
        stage();
        __syncthreads();
        if (k0 + D3P_GK < kend) fetch(k0 + D3P_GK);  // next slice in flight while this one multiplies
#pragma unroll
        for (int kk = 0; kk < D3P_GK; kk += 2) {
            const float a = As[kk + (lane >> 5)][wm * 32 + (lane & 31)];
            const float b = Bs[kk + (lane >> 5)][wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int col = n0 + wn * 32 + (lane & 31);
    if (col >= g.N) return;
    if (g.part) {  // split-K: raw partial tile, combined in fixed order by k_gemm_reduce
        float* out = g.part + (size_t)tz * g.M * g.N;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = m0 + wm * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
            if (row < g.M) out[(size_t)row * g.N + col] = acc[v];
        }
        return;
    }
    const float bv = g.bias ? g.bias[col + (col >= g.n_seg ? g.bias_njump : 0ll)] : 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int row = m0 + wm * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
        if (row < g.M) gemm_store(g, row, col, acc[v], bv);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// GEMM for the large products (operands 16-byte loadable): tile 128 (M) x 64 (N), K slices of 32, EIGHT wavefronts, each
// owning one 32 x 32 block of the tile (wavefront w: rows 32 (w & 3), columns 32 (w >> 2)).
//
// What bounds an fp32 GEMM on this chip (measured: tools/probes/mfma_probe.hip, mfma_valu_probe.hip, profiles/r02_mfma_*):
//   * v_mfma_f32_32x32x2_f32 sustains 155 TFLOP/s (27.1 ns per instruction and SIMD) from one wavefront per SIMD and one
//     accumulator chain;
//   * while an fp32 MFMA runs NOTHING else issues on its SIMD -- not a later instruction of the same wavefront, not a sibling
//     wavefront's VALU, LDS or memory instruction, whatever its priority.  The efficiency of a GEMM is therefore
//     MFMA cycles / (MFMA cycles + issue cycles of every other instruction on the SIMD + stalls nobody covers).
// Hence: (a) few instructions per MFMA -- fragments are read with ds_read_b128 (4 MFMA steps per read), operands are fetched
// with 16-byte loads whose addresses are a per-thread base + slice offset, edges are applied by selects at staging time;
// (b) two wavefronts per SIMD even when the tile count gives one workgroup per CU (224 tiles for 4096 x 400), so that one's
// waits (LDS round trip after the barrier, the barrier itself) are covered by the other's MFMAs; (c) one barrier per slice,
// placed in the MIDDLE of the slice's MFMAs: 8 MFMAs | stage slice i + 1, fetch slice i + 3 | barrier | read the fragments
// of slice i + 1 | 8 MFMAs -- the fragment reads land during the second half.
// (Tried and measured slower: 4 wavefronts of 32 x 64 with one workgroup per CU, 40-57 TFLOP/s; a ping-pong of two wavefront
// groups alternating between MFMA and memory phases, 35-44: the memory phase cannot run beside the MFMA phase.)
//
// LDS layout [row][k], k fastest, row stride 36 floats.  The MFMA step t of a slice multiplies columns {t, 16 + t} (any pairing
// of the 32 k's gives the same sum), so lane (r, h) needs k = 16 h .. 16 h + 15 of its row: four ds_read_b128 per operand.
// An operand that is k-fast in memory is stored as loaded (b128).  A row-fast one (float4 = 4 rows at one k) is transposed in
// registers where the thread holds two k's (A: 4 x b64 stores) and by four b32 stores otherwise (B).
// Loads are straight-line from CLAMPED addresses, the edges are applied to the LOADED values at staging time (guarded loads -- also
// "valid ? load : fill", which LLVM turns back into a branch -- make the compiler wait with vmcnt(0): no prefetch):
//   * k beyond the split's range: A is 0 there, and so is a k-fast B (selects: whatever the over-read padding holds, NaN and Inf
//     included, stays out; an n-fast B is read from clamped rows of the matrix itself);
//   * rows of A beyond m_real: 0, or 1 for the virtual row of ones (selects again); rows >= M / columns >= N only feed
//     accumulator entries that are never stored.
// The host guarantees N % 4 == 0 for an n-fast B (a float4 is inside or outside whole) and, for an m-fast A, a row stride of at
// least roundup4(m_real) (the last float4 may hold up to three rows past m_real, masked one by one).
// AK: A is k-fast (a_sk == 1), otherwise m-fast (a_sm == 1); BN: B is n-fast (b_sn == 1), otherwise k-fast (b_sk == 1).
// ------------------------------------------------------------------------------------------------------------------
#define D3P_GLD (D3P_GKB + 4)
// an element of A at an edge: the loaded value where the row exists in memory and k lies inside the split's range, `fill` (1 for the
// virtual row of ones, else 0) in a row that does not, 0 beyond the K range -- selected, never multiplied: the over-read padding
// (header above) may hold NaN or Inf, and 0 * Inf would poison the row
__device__ __forceinline__ float edge_sel(bool in_k, bool keep, float v, float fill) { return in_k ? (keep ? v : fill) : 0.f; }
template <bool AK, bool BN>
__global__ void __launch_bounds__(512) k_gemm_f32_w8(GemmArgs g)
{
    __shared__ __attribute__((aligned(16))) float As[2][D3P_GTM][D3P_GLD];  // [m][k]
    __shared__ __attribute__((aligned(16))) float Bs[2][D3P_GT][D3P_GLD];   // [n][k]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), grp = wave >> 2, wr = wave & 3;
    int tx, ty, tz;
    xcd_tile(tx, ty, tz);
    const int m0 = ty * D3P_GTM, n0 = tx * D3P_GT;
    const int kbeg = tz * g.k_per, kend = (kbeg + g.k_per < g.K) ? kbeg + g.k_per : g.K;
    const int m_real = g.a_last_one ? g.M - 1 : g.M;  // rows of A that exist in memory
    float16v acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;

    // ---- this thread's share of a slice: two float4 of A, one of B (row / k offsets inside the tile and slice)
    int a_m[2], a_k[2], b_n, b_k;
    if (AK) {
#pragma unroll
        for (int r = 0; r < 2; ++r) { const int f = tid + 512 * r; a_m[r] = f >> 3; a_k[r] = 4 * (f & 7); }
    } else {  // rows 4 mg .. 4 mg + 3 at k = 2 kp, 2 kp + 1
        const int mg = (tid & 7) + 8 * (tid >> 7), kp = (tid >> 3) & 15;
        a_m[0] = a_m[1] = 4 * mg;
        a_k[0] = 2 * kp;
        a_k[1] = 2 * kp + 1;
    }
    if (BN) { b_n = 4 * ((tid & 7) + 8 * (tid >> 8)); b_k = (tid >> 3) & 31; } else { b_n = tid >> 3; b_k = 4 * (tid & 7); }
    // Source addresses: per-thread 32-bit element offsets inside (tile rows, slice) -- rows clamped into the matrix -- on top of a
    // wavefront-uniform slice base that the scalar unit advances.  The two uniform conditions below select the cheap paths: a
    // slice that lies inside [0, K) whole is fetched from base + offset (no per-thread arithmetic; the few slices that straddle
    // K or lie beyond it -- the tail and the prefetches past the end -- clamp k per thread), and a tile that touches neither the
    // last rows of A nor the end of the split's K range is staged as loaded.
    // (K need not be a multiple of 4: the last float4 of a k-fast operand then runs past K inside its row -- the host checks the row
    // stride -- and both operands are masked element by element there)
    const int K4 = (g.K + 3) & ~3;
    const int ka_last = AK ? K4 - 4 : g.K - 1, kb_last = BN ? g.K - 1 : K4 - 4;
    // (m-fast A: the last float4 that holds real rows starts at roundup4(m_real) - 4; it may run up to 3 rows past m_real inside the
    // row stride -- the host checks a_sk >= roundup4(m_real) -- and those rows are masked one by one)
    const int m_last = AK ? m_real - 1 : ((m_real + 3) & ~3) - 4, n_last = g.N - (BN ? 4 : 1);
    // (a tile that holds nothing but the virtual row of ones -- m_real a multiple of the tile -- starts BEHIND the last row in memory:
    // every row clamps to m_last, below m0, so the base moves there too and the 32-bit offsets stay >= 0; as n_base for B below)
    const int m_base = m0 < m_last ? m0 : m_last;
    const long long a_kstride = AK ? 1 : g.a_sk, b_kstride = BN ? g.b_sk : 1;
    long long a_row[2];  // element offset of this thread's (clamped) row(s), k = 0
    unsigned a_off[2];   // ... + its k offset inside a slice, relative to the slice base
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int gm = m0 + a_m[r], cm = gm < m_last ? gm : m_last;
        a_row[r] = AK ? (long long)cm * g.a_sm : (long long)cm;
        a_off[r] = (unsigned)(a_row[r] - (AK ? (long long)m_base * g.a_sm : (long long)m_base) + (long long)a_k[r] * a_kstride);
    }
    const float* a_tile = g.A + (AK ? (long long)m_base * g.a_sm : (long long)m_base);  // uniform; offsets stay >= 0 (m_base above)
    const int gn_c = (n0 + b_n) < n_last ? (n0 + b_n) : n_last;
    const long long b_row = BN ? (long long)gn_c : (long long)gn_c * g.b_sn;
    // (a clamped column can lie left of the tile's first column only when the tile starts within 3 of N: then the base is moved)
    const int n_base = n0 < n_last ? n0 : n_last;
    const float* b_tile = g.B + (BN ? (long long)n_base : (long long)n_base * g.b_sn);
    const unsigned b_off = (unsigned)(b_row - (BN ? (long long)n_base : (long long)n_base * g.b_sn) + (long long)b_k * b_kstride);
    const bool m_edge = m0 + D3P_GTM > m_real;  // uniform: some rows of the tile are virtual (ones row) or absent
    // edge factors (constant over the slices): keep = 1 for a row that exists in memory, one = 1 for the virtual row of ones (row
    // m_real when a_last_one).  k-fast A: a float4 is one row (two rows per thread); m-fast A: four rows gm .. gm + 3, the same for
    // both of the thread's float4s.
    const int gm_a0 = m0 + a_m[0], gm_a1 = m0 + a_m[1];
    auto keep_of = [&](int row) { return row < m_real ? 1.f : 0.f; };
    auto one_of = [&](int row) { return (g.a_last_one && row == m_real) ? 1.f : 0.f; };
    const float kp0 = keep_of(gm_a0), kp1 = AK ? keep_of(gm_a1) : keep_of(gm_a0 + 1), kp2 = keep_of(gm_a0 + 2), kp3 = keep_of(gm_a0 + 3);
    const float on0 = one_of(gm_a0), on1 = AK ? one_of(gm_a1) : one_of(gm_a0 + 1), on2 = one_of(gm_a0 + 2), on3 = one_of(gm_a0 + 3);

    // (separate variables, not arrays: an array of float4 written on two paths was promoted to LDS by the compiler)
    float4 ra00, ra01, rb0, ra10, ra11, rb1;
    // Register set S fetches the slices S, S + 2, S + 4, ... of the split: its slice base pointers and k advance by two slices per
    // use (two scalar adds each -- a 64-bit k0 * stride product per fetch cost a dozen scalar instructions, and on this chip
    // they too wait for the MFMA in flight).
    const long long a_step2 = 2ll * D3P_GKB * a_kstride, b_step2 = 2ll * D3P_GKB * b_kstride;
    int fk[2] = {kbeg, kbeg + D3P_GKB};
    const float* fa[2] = {a_tile + (long long)kbeg * a_kstride, a_tile + (long long)(kbeg + D3P_GKB) * a_kstride};
    const float* fb[2] = {b_tile + (long long)kbeg * b_kstride, b_tile + (long long)(kbeg + D3P_GKB) * b_kstride};
    auto fetch = [&](auto S) {  // the set's next slice -> register set S; exactly three loads on either path
        constexpr int s = decltype(S)::value;
        float4 &a0 = s ? ra10 : ra00, &a1 = s ? ra11 : ra01, &bb = s ? rb1 : rb0;
        const int k0 = fk[s];
        if (k0 + D3P_GKB <= g.K) {
            a0 = *reinterpret_cast<const float4*>(fa[s] + a_off[0]);
            a1 = *reinterpret_cast<const float4*>(fa[s] + a_off[1]);
            bb = *reinterpret_cast<const float4*>(fb[s] + b_off);
        } else {
            const int gk0 = k0 + a_k[0], gk1 = k0 + a_k[1], gkb = k0 + b_k;
            a0 = *reinterpret_cast<const float4*>(g.A + a_row[0] + (long long)(gk0 < ka_last ? gk0 : ka_last) * a_kstride);
            a1 = *reinterpret_cast<const float4*>(g.A + a_row[1] + (long long)(gk1 < ka_last ? gk1 : ka_last) * a_kstride);
            bb = *reinterpret_cast<const float4*>(g.B + b_row + (long long)(gkb < kb_last ? gkb : kb_last) * b_kstride);
        }
        fk[s] = k0 + 2 * D3P_GKB;
        fa[s] += a_step2;
        fb[s] += b_step2;
    };
    auto stage = [&](auto S, int buf, int k0) {  // register set S (slice starting at k0) -> LDS buffer, edges applied
        constexpr int s = decltype(S)::value;
        float4 bb = s ? rb1 : rb0;
        float4 o[2] = {s ? ra10 : ra00, s ? ra11 : ra01};
        if (m_edge || k0 + D3P_GKB > kend) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const bool in_k = k0 + a_k[r] < kend;
                const float4 v = o[r];
                if (AK) {  // one row, four k's per float4: thread rows gm_a0 (r = 0), gm_a1 (r = 1)
                    const bool keep = (r ? kp1 : kp0) != 0.f;
                    const float fill = r ? on1 : on0;
                    const int kq = k0 + a_k[r];
                    o[r] = make_float4(edge_sel(kq + 0 < kend, keep, v.x, fill), edge_sel(kq + 1 < kend, keep, v.y, fill),
                                       edge_sel(kq + 2 < kend, keep, v.z, fill), edge_sel(kq + 3 < kend, keep, v.w, fill));
                } else {   // four rows per float4
                    o[r] = make_float4(edge_sel(in_k, kp0 != 0.f, v.x, on0), edge_sel(in_k, kp1 != 0.f, v.y, on1),
                                       edge_sel(in_k, kp2 != 0.f, v.z, on2), edge_sel(in_k, kp3 != 0.f, v.w, on3));
                }
            }
            if (!BN) {   // a k-fast B: its last float4 may run past K inside the row, and what lies there need not be finite
                const int kq = k0 + b_k;
                bb = make_float4(kq + 0 < kend ? bb.x : 0.f, kq + 1 < kend ? bb.y : 0.f, kq + 2 < kend ? bb.z : 0.f, kq + 3 < kend ? bb.w : 0.f);
            }
        }
        if (AK) {
            *reinterpret_cast<float4*>(&As[buf][a_m[0]][a_k[0]]) = o[0];
            *reinterpret_cast<float4*>(&As[buf][a_m[1]][a_k[1]]) = o[1];
        } else {  // 2 k x 4 rows, transposed in registers
            *reinterpret_cast<float2*>(&As[buf][a_m[0] + 0][a_k[0]]) = make_float2(o[0].x, o[1].x);
            *reinterpret_cast<float2*>(&As[buf][a_m[0] + 1][a_k[0]]) = make_float2(o[0].y, o[1].y);
            *reinterpret_cast<float2*>(&As[buf][a_m[0] + 2][a_k[0]]) = make_float2(o[0].z, o[1].z);
            *reinterpret_cast<float2*>(&As[buf][a_m[0] + 3][a_k[0]]) = make_float2(o[0].w, o[1].w);
        }
        if (BN) {
            Bs[buf][b_n + 0][b_k] = bb.x;
            Bs[buf][b_n + 1][b_k] = bb.y;
            Bs[buf][b_n + 2][b_k] = bb.z;
            Bs[buf][b_n + 3][b_k] = bb.w;
        } else {
            *reinterpret_cast<float4*>(&Bs[buf][b_n][b_k]) = bb;
        }
    };
    struct Frag { float4 a[4], b[4]; };
    const int fr = lane & 31, fh = lane >> 5;
    auto read_frags = [&](int buf, Frag& f) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f.a[q] = *reinterpret_cast<const float4*>(&As[buf][32 * wr + fr][16 * fh + 4 * q]);
            f.b[q] = *reinterpret_cast<const float4*>(&Bs[buf][32 * grp + fr][16 * fh + 4 * q]);
        }
    };
    auto mma_half = [&](const Frag& f, int half) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 a = f.a[2 * half + q], b = f.b[2 * half + q];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    const int KB = D3P_GKB;
    // Slice i lives in LDS buffer i & 1; at the top of iteration i the register set (i + 1) & 1 holds slice i + 1 and the set i & 1
    // slice i + 2 (both possibly still in flight) and f0 the fragments of slice i.  A buffer is rewritten one barrier after its last
    // reader issued (and completed) its reads, and read after the barrier that follows its writes.
    // (the slice count is rounded up to even: the register-set indices stay compile-time constants; empty slices multiply zeros)
    Frag f0, f1;
    fetch(S0{});
    fetch(S1{});
    stage(S0{}, 0, kbeg);
    fetch(S0{});
    __syncthreads();
    read_frags(0, f0);
    const int ns = (kend - kbeg + KB - 1) / KB;
    for (int i = 0; i < ns; i += 2) {
        const int k_i = kbeg + i * KB;
        mma_half(f0, 0);
        stage(S1{}, 1, k_i + KB);
        fetch(S1{});
        __syncthreads();
        read_frags(1, f1);
        mma_half(f0, 1);
        __builtin_amdgcn_sched_barrier(0);
        mma_half(f1, 0);
        stage(S0{}, 0, k_i + 2 * KB);
        fetch(S0{});
        __syncthreads();
        read_frags(0, f0);
        mma_half(f1, 1);
        __builtin_amdgcn_sched_barrier(0);
    }
    const int col = n0 + 32 * grp + (lane & 31);
    if (col >= g.N) return;
    if (g.part) {  // split-K: raw partial tile, combined in fixed order by the consumer
        float* out = g.part + (size_t)tz * g.M * g.N;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = m0 + wr * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
            if (row < g.M) out[(size_t)row * g.N + col] = acc[v];
        }
        return;
    }
    const float bv = g.bias ? g.bias[col + (col >= g.n_seg ? g.bias_njump : 0ll)] : 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int row = m0 + wr * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
        if (row < g.M) gemm_store(g, row, col, acc[v], bv);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// The same product on the bf16 matrix pipe at fp32 accuracy (round 3): every fp32 operand element is split EXACTLY into three
// bf16 parts (x = x0 + x1 + x2: the top 8, the next 8 and the last 8 bits of its 24-bit significand -- truncations, so each
// remainder is exact), and the product a b is accumulated in fp32 as
//     a0 b0 + a0 b1 + a1 b0 + a0 b2 + a1 b1 + a2 b0
// -- six v_mfma_f32_32x32x16_bf16 per 16 k's.  Every partial product is exact (8 x 8 bits), the three dropped terms are below
// 2^-23 |a b| -- the size of ONE fp32 rounding of the product -- and the accumulation is the fp32 accumulation of the fp32 MFMA.
// Why: v_mfma_f32_32x32x2_f32 runs on the VECTOR pipe at 1/16 of the bf16 rate and nothing issues beside it (the 41 % ceiling of
// k_gemm_f32_w8); the bf16 matrix pipe does six of these MFMAs in 6/16 of the time AND lets the vector unit
// (which does the splitting: 5.5 instructions per element) and the LDS run beside it.
// Same tile (128 x 64, eight waves of 32 x 32, K slices of 32), same fetch path, edge handling and epilogue as k_gemm_f32_w8; the
// LDS holds three bf16 planes per operand, [plane][row][k] with k fastest and a row stride of 40 bf16 (80 bytes: the b128
// fragment reads of 16 consecutive rows fall into distinct 16-byte slots of a 256-byte bank row).
// ------------------------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
#define D3P_BLD 40   // row stride of a plane in bf16 elements
// Chunk swizzle of the planes (round 6): a row's K slice is four 16-byte chunks (8 bf16 each); row r keeps chunk c at position
// c ^ parity(r & 0x1c).  The fragment reads stay conflict-free (the ds_read_b128 lane groups still meet 16 distinct slots of the
// 256-byte bank row), and the staging stores of the m-fast A and n-fast B forms -- lanes 4 rows apart writing the same word of
// their rows, banks 16 r mod 32: 4-way, twice the LDS-array cycles (SQ_LDS_BANK_CONFLICT was 55 % of SQ_LDS_IDX_ACTIVE in the
// grouped weight-gradient launch, profiles/r06_vae_gemm_pmc.json) -- become 2-way, which a ds_write_b32 hides
// (MI355X_MICROARCH.md, LDS; the layouts were searched with the guide's bank model).
// (the unswizzled layout of rounds 3 - 5 as a build alternate: tools/experiments/r06_gemm_split_rne_and_unswizzled_planes.patch)
__device__ __forceinline__ int plane_swz(int row) { return (__builtin_popcount((unsigned)row & 0x1cu) & 1) << 3; }   // XOR into the k index
// DIAGNOSTIC builds only (tools/gemm_diag.sh compiles this file with -DD3P_GEMM_DIAG=<bits> into a library of its own; results are
// WRONG, only the time matters): 1 no splitting arithmetic (all planes = the top halves), 2 no global loads behind the first two
// slices, 4 no staging at all (no splitting, no LDS writes), 8 fragments read once, 16 no MFMAs.  0 = the product kernel.
#ifndef D3P_GEMM_DIAG
#define D3P_GEMM_DIAG 0
#endif
// the three bf16 parts of two fp32 values, as three words {part of x1 (high half) | part of x0 (low half)}: truncations (the top 8,
// the next 8 and the last 8 bits of the 24-bit significand), so each remainder is exact.  11 vector instructions per pair:
// 4 v_and, 4 v_sub (VOP2: 2.4 cycles each), 3 v_perm (4.3).
// ROUND-TO-NEAREST parts (round 6, built and measured, NOT adopted; tools/experiments/r06_gemm_split_rne_and_unswizzled_planes.patch):
// 9 instructions per pair (3 v_cvt_pk_bf16_f32 + 2 v_lshl + 2 v_and + 2 v_pk_add_f32) -- FEWER instructions (60 instead of 72 per wave
// and K slice) and SLOWER: h1 32.8 -> 34.3 us, the VAE update 249 -> 253.5 us on one box, alternating (profiles/r06_split_rne_ab.txt)
// -- the converting and the packed instructions issue at the VOP3 / packed rate or worse (profiles/r03_valu_opcodes.json: 4.3 cycles
// against 2.4), and beside the bf16 MFMAs issue time is what counts (docs/experiments_r06.md section 3).
__device__ __forceinline__ void split_pair(float x0, float x1, uint32_t& w0, uint32_t& w1, uint32_t& w2)
{
    const uint32_t u0 = __float_as_uint(x0), u1 = __float_as_uint(x1);
    w0 = __builtin_amdgcn_perm(u1, u0, 0x07060302u);
    if (D3P_GEMM_DIAG & 1) { w1 = w0; w2 = w0; return; }
    const float r0 = x0 - __uint_as_float(u0 & 0xffff0000u), r1 = x1 - __uint_as_float(u1 & 0xffff0000u);
    const uint32_t v0 = __float_as_uint(r0), v1 = __float_as_uint(r1);
    w1 = __builtin_amdgcn_perm(v1, v0, 0x07060302u);
    const float s0 = r0 - __uint_as_float(v0 & 0xffff0000u), s1 = r1 - __uint_as_float(v1 & 0xffff0000u);
    w2 = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
}

// one 128 x 64 tile (tx, ty) of K slab tz of the product g, by one 8-wave workgroup
template <bool AK, bool BN, bool EPI4 = false>
__device__ __forceinline__ void gemm_bf16x3_tile(const GemmArgs& g, const int tx, const int ty, const int tz)
{
    __shared__ __attribute__((aligned(16))) unsigned short Ap[2][3][D3P_GTM][D3P_BLD];  // [buffer][plane][m][k]
    __shared__ __attribute__((aligned(16))) unsigned short Bp[2][3][D3P_GT][D3P_BLD];   // [buffer][plane][n][k]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), grp = wave >> 2, wr = wave & 3;
    const int m0 = ty * D3P_GTM, n0 = tx * D3P_GT;
    const int kbeg = tz * g.k_per, kend = (kbeg + g.k_per < g.K) ? kbeg + g.k_per : g.K;
    const int m_real = g.a_last_one ? g.M - 1 : g.M;
    float16v acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    float xpre[EPI4 ? 16 : 1];   // EPI4: this lane's 16 elements of ep_x, in flight during the K loop
    if (EPI4) {
        const int pcol = n0 + 32 * grp + (lane & 31);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = m0 + wr * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
            const bool ok = pcol < g.N && row < g.M;
            xpre[v] = ok ? g.ep_x[(size_t)row * g.ldc + pcol] : 0.f;
        }
    }

    // ---- this thread's share of a slice (as in k_gemm_f32_w8): two float4 of A, one of B
    int a_m[2], a_k[2], b_n, b_k;
    if (AK) {
#pragma unroll
        for (int r = 0; r < 2; ++r) { const int f = tid + 512 * r; a_m[r] = f >> 3; a_k[r] = 4 * (f & 7); }
    } else {  // rows 4 mg .. 4 mg + 3 at k = 2 kp, 2 kp + 1
        const int mg = (tid & 7) + 8 * (tid >> 7), kp = (tid >> 3) & 15;
        a_m[0] = a_m[1] = 4 * mg;
        a_k[0] = 2 * kp;
        a_k[1] = 2 * kp + 1;
    }
    // n-fast B: columns 4 ng .. 4 ng + 3 at ONE k; lanes l and l ^ 8 hold k and k ^ 1 of the same columns (bit 3 of tid = bit 0 of k)
    if (BN) { b_n = 4 * ((tid & 7) + 8 * (tid >> 8)); b_k = (tid >> 3) & 31; } else { b_n = tid >> 3; b_k = 4 * (tid & 7); }
    // where this thread's share goes in the swizzled planes (plane_swz: rows 4 mg .. 4 mg + 3 share one swizzle, b_n likewise)
    const int a_kw[2] = {a_k[0] ^ plane_swz(a_m[0]), a_k[1] ^ plane_swz(a_m[1])};
    const int b_sw = plane_swz(b_n);
    const int K4 = (g.K + 3) & ~3;
    const int ka_last = AK ? K4 - 4 : g.K - 1, kb_last = BN ? g.K - 1 : K4 - 4;
    const int m_last = AK ? m_real - 1 : ((m_real + 3) & ~3) - 4, n_last = g.N - (BN ? 4 : 1);
    // (a tile that holds nothing but the virtual row of ones -- m_real a multiple of the tile -- starts BEHIND the last row in memory:
    // every row clamps to m_last, below m0, so the base moves there too and the 32-bit offsets stay >= 0; as n_base for B below)
    const int m_base = m0 < m_last ? m0 : m_last;
    const long long a_kstride = AK ? 1 : g.a_sk, b_kstride = BN ? g.b_sk : 1;
    long long a_row[2];
    unsigned a_off[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int gm = m0 + a_m[r], cm = gm < m_last ? gm : m_last;
        a_row[r] = AK ? (long long)cm * g.a_sm : (long long)cm;
        a_off[r] = (unsigned)(a_row[r] - (AK ? (long long)m_base * g.a_sm : (long long)m_base) + (long long)a_k[r] * a_kstride);
    }
    const float* a_tile = g.A + (AK ? (long long)m_base * g.a_sm : (long long)m_base);
    const int gn_c = (n0 + b_n) < n_last ? (n0 + b_n) : n_last;
    const long long b_row = BN ? (long long)gn_c : (long long)gn_c * g.b_sn;
    const int n_base = n0 < n_last ? n0 : n_last;
    const float* b_tile = g.B + (BN ? (long long)n_base : (long long)n_base * g.b_sn);
    const unsigned b_off = (unsigned)(b_row - (BN ? (long long)n_base : (long long)n_base * g.b_sn) + (long long)b_k * b_kstride);
    const bool m_edge = m0 + D3P_GTM > m_real;
    const int gm_a0 = m0 + a_m[0], gm_a1 = m0 + a_m[1];
    auto keep_of = [&](int row) { return row < m_real ? 1.f : 0.f; };
    auto one_of = [&](int row) { return (g.a_last_one && row == m_real) ? 1.f : 0.f; };
    const float kp0 = keep_of(gm_a0), kp1 = AK ? keep_of(gm_a1) : keep_of(gm_a0 + 1), kp2 = keep_of(gm_a0 + 2), kp3 = keep_of(gm_a0 + 3);
    const float on0 = one_of(gm_a0), on1 = AK ? one_of(gm_a1) : one_of(gm_a0 + 1), on2 = one_of(gm_a0 + 2), on3 = one_of(gm_a0 + 3);

    float4 ra00, ra01, rb0, ra10, ra11, rb1;
    float rs0 = 1.f, rs1 = 1.f;   // b_row_scale of this thread's row of B (BN), per register set
    const bool b_scaled = BN && g.b_row_scale != nullptr;
    const long long a_step2 = 2ll * D3P_GKB * a_kstride, b_step2 = 2ll * D3P_GKB * b_kstride;
    int fk[2] = {kbeg, kbeg + D3P_GKB};
    const float* fa[2] = {a_tile + (long long)kbeg * a_kstride, a_tile + (long long)(kbeg + D3P_GKB) * a_kstride};
    const float* fb[2] = {b_tile + (long long)kbeg * b_kstride, b_tile + (long long)(kbeg + D3P_GKB) * b_kstride};
    auto fetch = [&](auto S) {
        constexpr int s = decltype(S)::value;
        float4 &a0 = s ? ra10 : ra00, &a1 = s ? ra11 : ra01, &bb = s ? rb1 : rb0;
        const int k0 = fk[s];
        if ((D3P_GEMM_DIAG & 2) && k0 >= kbeg + 2 * D3P_GKB) { fk[s] = k0 + 2 * D3P_GKB; return; }
        if (b_scaled) {
            const int gk = k0 + b_k;
            (s ? rs1 : rs0) = g.b_row_scale[gk < g.K ? gk : g.K - 1];
        }
        if (k0 + D3P_GKB <= g.K) {
            a0 = *reinterpret_cast<const float4*>(fa[s] + a_off[0]);
            a1 = *reinterpret_cast<const float4*>(fa[s] + a_off[1]);
            bb = *reinterpret_cast<const float4*>(fb[s] + b_off);
        } else {
            const int gk0 = k0 + a_k[0], gk1 = k0 + a_k[1], gkb = k0 + b_k;
            a0 = *reinterpret_cast<const float4*>(g.A + a_row[0] + (long long)(gk0 < ka_last ? gk0 : ka_last) * a_kstride);
            a1 = *reinterpret_cast<const float4*>(g.A + a_row[1] + (long long)(gk1 < ka_last ? gk1 : ka_last) * a_kstride);
            bb = *reinterpret_cast<const float4*>(g.B + b_row + (long long)(gkb < kb_last ? gkb : kb_last) * b_kstride);
        }
        fk[s] = k0 + 2 * D3P_GKB;
        fa[s] += a_step2;
        fb[s] += b_step2;
    };
    // EDGE = false: the slice lies inside [kbeg, kend) and the tile inside the rows of A that exist -- no edge arithmetic, no branch
    // (the steady state: its body is straight-line code that the scheduler interleaves with the MFMAs of the slice before)
    auto stage = [&](auto S, int buf, int k0, auto EDGE, auto A1P) {  // register set S (slice starting at k0): edges applied, split, three planes -> LDS
        constexpr int s = decltype(S)::value;
        constexpr bool A1 = decltype(A1P)::value;   // A is exactly bf16: plane 0 alone
        if ((D3P_GEMM_DIAG & 4) && k0 >= kbeg + 2 * D3P_GKB) return;
        float4 bb = s ? rb1 : rb0;
        if (BN) { const float c = s ? rs1 : rs0; bb = make_float4(bb.x * c, bb.y * c, bb.z * c, bb.w * c); }
        float4 o[2] = {s ? ra10 : ra00, s ? ra11 : ra01};
        if (decltype(EDGE)::value && (m_edge || k0 + D3P_GKB > kend)) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const bool in_k = k0 + a_k[r] < kend;
                const float4 v = o[r];
                if (AK) {
                    const bool keep = (r ? kp1 : kp0) != 0.f;
                    const float fill = r ? on1 : on0;
                    const int kq = k0 + a_k[r];
                    o[r] = make_float4(edge_sel(kq + 0 < kend, keep, v.x, fill), edge_sel(kq + 1 < kend, keep, v.y, fill),
                                       edge_sel(kq + 2 < kend, keep, v.z, fill), edge_sel(kq + 3 < kend, keep, v.w, fill));
                } else {
                    o[r] = make_float4(edge_sel(in_k, kp0 != 0.f, v.x, on0), edge_sel(in_k, kp1 != 0.f, v.y, on1),
                                       edge_sel(in_k, kp2 != 0.f, v.z, on2), edge_sel(in_k, kp3 != 0.f, v.w, on3));
                }
            }
            if (!BN) {   // a k-fast B: its last float4 may run past K inside the row, and what lies there need not be finite
                const int kq = k0 + b_k;
                bb = make_float4(kq + 0 < kend ? bb.x : 0.f, kq + 1 < kend ? bb.y : 0.f, kq + 2 < kend ? bb.z : 0.f, kq + 3 < kend ? bb.w : 0.f);
            }
        }
        uint32_t w[3];
        auto top16 = [](float x0, float x1) { return __builtin_amdgcn_perm(__float_as_uint(x1), __float_as_uint(x0), 0x07060302u); };
        if (AK) {  // one row, four consecutive k's per float4: two words per plane, one 8-byte store
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (A1) {
                    *reinterpret_cast<uint2*>(&Ap[buf][0][a_m[r]][a_kw[r]]) = make_uint2(top16(o[r].x, o[r].y), top16(o[r].z, o[r].w));
                } else {
                    uint32_t x[3], y[3];
                    split_pair(o[r].x, o[r].y, x[0], x[1], x[2]);
                    split_pair(o[r].z, o[r].w, y[0], y[1], y[2]);
#pragma unroll
                    for (int p = 0; p < 3; ++p) *reinterpret_cast<uint2*>(&Ap[buf][p][a_m[r]][a_kw[r]]) = make_uint2(x[p], y[p]);
                }
            }
        } else {   // four rows at k = 2 kp (o[0]) and 2 kp + 1 (o[1]): one word per row and plane
            const float lo4[4] = {o[0].x, o[0].y, o[0].z, o[0].w}, hi4[4] = {o[1].x, o[1].y, o[1].z, o[1].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (A1) {
                    *reinterpret_cast<uint32_t*>(&Ap[buf][0][a_m[0] + i][a_kw[0]]) = top16(lo4[i], hi4[i]);
                } else {
                    split_pair(lo4[i], hi4[i], w[0], w[1], w[2]);
#pragma unroll
                    for (int p = 0; p < 3; ++p) *reinterpret_cast<uint32_t*>(&Ap[buf][p][a_m[0] + i][a_kw[0]]) = w[p];
                }
            }
        }
        if (BN) {  // four columns at one k; the lane 8 away holds k ^ 1: the even-k lane takes columns 0, 1, the odd-k lane 2, 3
            const bool odd = (b_k & 1) != 0;
            const float give0 = odd ? bb.x : bb.z, give1 = odd ? bb.y : bb.w;   // what the partner needs from this lane
            const float got0 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(give0), 0x128, 0xF, 0xF, false));  // row_ror:8
            const float got1 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(give1), 0x128, 0xF, 0xF, false));
            // this lane's two columns at (k even, k odd)
            const float e0 = odd ? got0 : bb.x, o0 = odd ? bb.z : got0, e1 = odd ? got1 : bb.y, o1 = odd ? bb.w : got1;
            const int nn = b_n + (odd ? 2 : 0), kk = (b_k & ~1) ^ b_sw;   // (rows nn, nn + 1 lie in b_n's group of four: one swizzle)
            split_pair(e0, o0, w[0], w[1], w[2]);
#pragma unroll
            for (int p = 0; p < 3; ++p) *reinterpret_cast<uint32_t*>(&Bp[buf][p][nn][kk]) = w[p];
            split_pair(e1, o1, w[0], w[1], w[2]);
#pragma unroll
            for (int p = 0; p < 3; ++p) *reinterpret_cast<uint32_t*>(&Bp[buf][p][nn + 1][kk]) = w[p];
        } else {
            uint32_t x[3], y[3];
            split_pair(bb.x, bb.y, x[0], x[1], x[2]);
            split_pair(bb.z, bb.w, y[0], y[1], y[2]);
#pragma unroll
            for (int p = 0; p < 3; ++p) *reinterpret_cast<uint2*>(&Bp[buf][p][b_n][b_k ^ b_sw]) = make_uint2(x[p], y[p]);
        }
    };
    struct Frag { bf16x8 a[2][3], b[2][3]; };   // [k step of 16][plane]
    const int fr = lane & 31, fh = lane >> 5;
    const int f_sw = plane_swz(fr);   // (the wave's rows 32 wr + fr / 32 grp + fr: bits 2 - 4 are fr's)
    bool frags_read = false;
    auto read_frags = [&](int buf, Frag& f, auto A1P) {
        constexpr bool A1 = decltype(A1P)::value;
        if (D3P_GEMM_DIAG & 8) { if (frags_read) return; frags_read = true; }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                if (!A1 || p == 0)
                    f.a[ks][p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(&Ap[buf][p][32 * wr + fr][(16 * ks + 8 * fh) ^ f_sw]));
                f.b[ks][p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(&Bp[buf][p][32 * grp + fr][(16 * ks + 8 * fh) ^ f_sw]));
            }
    };
    auto mma_half = [&](const Frag& f, int ks, auto A1P) {   // smallest terms first
        constexpr bool A1 = decltype(A1P)::value;
        if (D3P_GEMM_DIAG & 16) return;
        if (!A1) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[ks][2], f.b[ks][0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[ks][0], f.b[ks][2], acc, 0, 0, 0);
        if (!A1) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[ks][1], f.b[ks][1], acc, 0, 0, 0);
        if (!A1) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[ks][1], f.b[ks][0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[ks][0], f.b[ks][1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[ks][0], f.b[ks][0], acc, 0, 0, 0);
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    const int KB = D3P_GKB;
    using EdgeY = std::true_type;
    using EdgeN = std::false_type;
    auto main_loop = [&](auto A1P) {
    constexpr bool A1 = decltype(A1P)::value;
    Frag f0, f1;
    fetch(S0{});
    fetch(S1{});
    stage(S0{}, 0, kbeg, EdgeY{}, A1P);
    fetch(S0{});
    __syncthreads();
    read_frags(0, f0, A1P);
    if (D3P_GEMM_DIAG & 8) f1 = f0;
    const int ns = (kend - kbeg + KB - 1) / KB;
    // one MFMA, then a share of the other work of the same half slice: the bf16 matrix pipe runs beside the vector unit and the LDS,
    // but only what stands BETWEEN two MFMAs in a wave's instruction stream can run beside them
#define D3P_MIX_VALU 12
#define D3P_MIX_STAGE()                                                                                     \
    _Pragma("unroll") for (int q_ = 0; q_ < 6; ++q_) {                                                      \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  /* 1 MFMA */                                    \
        __builtin_amdgcn_sched_group_barrier(0x002, D3P_MIX_VALU, 0); /* the splitting's vector instructions */ \
        __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);  /* 2 LDS writes */                              \
    }
#define D3P_MIX_READ()                                                                                      \
    _Pragma("unroll") for (int q_ = 0; q_ < 6; ++q_) {                                                      \
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  /* 2 LDS reads */                               \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  /* 1 MFMA */                                    \
    }
#define D3P_MIX_STAGE_A1()                                                                                  \
    _Pragma("unroll") for (int q_ = 0; q_ < 3; ++q_) {                                                      \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  /* 1 MFMA */                                    \
        __builtin_amdgcn_sched_group_barrier(0x002, 10, 0); /* 10 VALU (splitting B, packing A) */          \
        __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);  /* 2 LDS writes */                              \
    }
#define D3P_MIX_READ_A1()                                                                                   \
    _Pragma("unroll") for (int q_ = 0; q_ < 3; ++q_) {                                                      \
        __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);  /* 3 LDS reads */                               \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  /* 1 MFMA */                                    \
    }
    for (int i = 0; i < ns; i += 2) {
        const int k_i = kbeg + i * KB;
        if (!m_edge && k_i + 3 * KB <= kend) {   // both slices staged in this iteration are whole: the branch-free body
            mma_half(f0, 0, A1P);
            stage(S1{}, 1, k_i + KB, EdgeN{}, A1P);
            if (A1) { D3P_MIX_STAGE_A1() } else { D3P_MIX_STAGE() }
            fetch(S1{});
            __syncthreads();
            read_frags(1, f1, A1P);
            mma_half(f0, 1, A1P);
            if (A1) { D3P_MIX_READ_A1() } else { D3P_MIX_READ() }
            __builtin_amdgcn_sched_barrier(0);
            mma_half(f1, 0, A1P);
            stage(S0{}, 0, k_i + 2 * KB, EdgeN{}, A1P);
            if (A1) { D3P_MIX_STAGE_A1() } else { D3P_MIX_STAGE() }
            fetch(S0{});
            __syncthreads();
            read_frags(0, f0, A1P);
            mma_half(f1, 1, A1P);
            if (A1) { D3P_MIX_READ_A1() } else { D3P_MIX_READ() }
            __builtin_amdgcn_sched_barrier(0);
        } else {
            mma_half(f0, 0, A1P);
            stage(S1{}, 1, k_i + KB, EdgeY{}, A1P);
            fetch(S1{});
            __syncthreads();
            read_frags(1, f1, A1P);
            mma_half(f0, 1, A1P);
            mma_half(f1, 0, A1P);
            stage(S0{}, 0, k_i + 2 * KB, EdgeY{}, A1P);
            fetch(S0{});
            __syncthreads();
            read_frags(0, f0, A1P);
            mma_half(f1, 1, A1P);
        }
    }
#undef D3P_MIX_STAGE_A1
#undef D3P_MIX_READ_A1
    };
    // (wave-uniform: the flag is one word for the whole product)
    if (g.a_exact16 && (uint32_t)__builtin_amdgcn_readfirstlane((int)*g.a_exact16) != g.a_exact_nonce) main_loop(std::true_type{});
    else main_loop(std::false_type{});
#undef D3P_MIX_STAGE
#undef D3P_MIX_READ
    const int col = n0 + 32 * grp + (lane & 31);
    if (EPI4) {   // (every lane stays for the row sums: a column beyond N contributes zeros)
        const bool col_ok = col < g.N;
        const float bv = (g.bias && col_ok) ? g.bias[col] : 0.f;
        float ll[16], xx[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = m0 + wr * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
            const bool ok = col_ok && row < g.M;
            const float o = __fmaf_rn(g.alpha, acc[v], bv), x = xpre[v];
            // one exponential per element, as in k_vae_out: en = exp(-|o|); softplus(o) = max(o, 0) + log(1 + en)
            const float en = __expf(-fabsf(o)), r = __builtin_amdgcn_rcpf(1.0f + en);
            if (ok) g.C[(size_t)row * g.ldc + col] = g.ex_sc * ((o >= 0.0f ? r : en * r) - x);
            ll[v] = ok ? x * o - (fmaxf(o, 0.0f) + __logf(1.0f + en)) : 0.f;
            xx[v] = x * x;
        }
        // sums over the 32 columns of each half wave (lanes 0 - 31: rows + 0, lanes 32 - 63: rows + 4): four DPP steps inside the rows
        // of 16 lanes, row_bcast:15 adds row 0 into row 1 and row 2 into row 3 -- lanes 31 and 63 hold the half sums
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            float a_ = ll[v], b_ = xx[v];
            a_ += dpp_mov<0xB1>(a_); b_ += dpp_mov<0xB1>(b_);
            a_ += dpp_mov<0x4E>(a_); b_ += dpp_mov<0x4E>(b_);
            a_ += dpp_mov<0x141>(a_); b_ += dpp_mov<0x141>(b_);
            a_ += dpp_mov<0x140>(a_); b_ += dpp_mov<0x140>(b_);
            asm("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                "v_add_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1"
                : "+v"(a_), "+v"(b_));
            ll[v] = a_; xx[v] = b_;
        }
        if ((lane & 31) == 31 && n0 + 32 * grp < g.N) {
            const int cg = (n0 >> 5) + grp;   // this wave's group of 32 columns
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = m0 + wr * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
                if (row < g.M) {
                    g.ep_ll[(size_t)cg * g.M + row] = ll[v];
                    g.ep_xx[(size_t)cg * g.M + row] = xx[v];
                }
            }
        }
        return;
    }
    if (col >= g.N) return;
    if (g.part) {
        float* out = g.part + (size_t)tz * g.M * g.N;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = m0 + wr * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
            if (row < g.M) out[(size_t)row * g.N + col] = acc[v];
        }
        return;
    }
    const float bv = g.bias ? g.bias[col + (col >= g.n_seg ? g.bias_njump : 0ll)] : 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int row = m0 + wr * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
        if (row < g.M) gemm_store(g, row, col, acc[v], bv);
    }
}

template <bool AK, bool BN, bool EPI4 = false>
__global__ void __launch_bounds__(512) k_gemm_bf16x3(GemmArgs g)
{
    int tx, ty, tz;
    xcd_tile(tx, ty, tz);
    gemm_bf16x3_tile<AK, BN, EPI4>(g, tx, ty, tz);
}

// several products in one launch (GemmGroup, d3p_gemm.h)
template <bool AK, bool BN>
__global__ void __launch_bounds__(512) k_gemm_bf16x3_group(GemmGroup q)
{
    if (q.sum_in && blockIdx.x == 0) {   // (workgroup-uniform; the FIRST workgroup: dealt out last it would be the launch's tail)
        __shared__ float part[512];
        float sm = 0.f;
        for (unsigned i = threadIdx.x; i < q.sum_n; i += 512) sm += q.sum_in[i];
        part[threadIdx.x] = sm;
        __syncthreads();
        for (int off = 256; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) *q.sum_out = part[0];
        return;
    }
    const unsigned bid = blockIdx.x - (q.sum_in ? 1u : 0u);
    const unsigned c = bid & 7u, j = bid >> 3;
    int p = 0;
#pragma unroll
    for (int k = 1; k < D3P_GROUP_MAX; ++k) p += (j >= q.slot[k]) ? 1 : 0;
    const unsigned R = c * (q.slot[p + 1] - q.slot[p]) + (j - q.slot[p]);
    if (R >= q.cnt[p]) return;
    const unsigned gx = q.gx[p], gy = q.gy[p];
    gemm_bf16x3_tile<AK, BN>(q.g[p], (int)(R % gx), (int)((R / gx) % gy), (int)(R / (gx * gy)));
}

// the instantiation KERNEL<x, y> of two run-time flags (<AK, BN> / <VA, VB>), launched
#define D3P_LAUNCH_XY(KERNEL, x, y, grid, block, s, arg)                                   \
    do {                                                                                   \
        if ((x) && (y)) hipLaunchKernelGGL((KERNEL<true, true>), grid, block, 0, s, arg);  \
        else if (x) hipLaunchKernelGGL((KERNEL<true, false>), grid, block, 0, s, arg);     \
        else if (y) hipLaunchKernelGGL((KERNEL<false, true>), grid, block, 0, s, arg);     \
        else hipLaunchKernelGGL((KERNEL<false, false>), grid, block, 0, s, arg);           \
    } while (0)

int gemm_group_launch(hipStream_t s, GemmGroupPlan& G)
{
    if (G.n == 0) return D3P_OK;
    unsigned slots = 0;
    for (int p = 0; p < D3P_GROUP_MAX; ++p) {
        G.q.slot[p] = slots;
        if (p < G.n) slots += (G.q.cnt[p] + 7u) / 8u;
        else { G.q.cnt[p] = 0; G.q.gx[p] = G.q.gy[p] = 1; G.q.g[p] = G.q.g[0]; }
    }
    G.q.slot[D3P_GROUP_MAX] = slots;
    G.q.sum_in = G.sum_in; G.q.sum_out = G.sum_out; G.q.sum_n = G.sum_n;
    const dim3 grid(8u * slots + (G.sum_in ? 1u : 0u));
    D3P_LAUNCH_XY(k_gemm_bf16x3_group, G.ak, G.bn, grid, dim3(512), s, G.q);
    G.n = 0;
    return check_launch("k_gemm_bf16x3_group");
}

// Split count of a k_gemm_bf16x3 product, or ONE count for all members of a group (they share K = the batch): the one whose rounds
// of one workgroup per CU (92 KB of LDS each) cost least, a round costing its K range plus about two slices of prologue and
// epilogue.  tiles = 128 x 64 tiles of the product, or of all members together.
// can gemm_group_splits return sp for a K range?  The rounded K range reproduces the count and a range holds two slices or more.
static bool gemm_split_count_ok(int sp, int K, int* k_per = nullptr, int* n_slabs = nullptr)
{
    if (sp < 1 || sp > D3P_WPART_SPLITS) return false;
    int kp = (K + sp - 1) / sp;
    kp = (kp + D3P_GKB - 1) / D3P_GKB * D3P_GKB;
    const int ns = (K + kp - 1) / kp;
    if (k_per) *k_per = kp;
    if (n_slabs) *n_slabs = ns;
    return ns == sp && kp >= 2 * D3P_GKB;
}

int gemm_group_splits(unsigned tiles, int K)
{
    static const int n_cu = [] {   // (one process drives one device: d3p_amd.dist; initialised once, thread-safely)
        int dev = 0, n = 0;
        const bool ok = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0;
        if (!ok) (void)hipGetLastError();
        return ok ? n : 256;
    }();
    int best = 1;
    double best_cost = 1e30;
    for (int sp = 1; sp <= D3P_WPART_SPLITS; ++sp) {
        int kp = 0, ns = 0;
        if (!gemm_split_count_ok(sp, K, &kp, &ns)) continue;
        const double rounds = std::ceil((double)tiles * ns / n_cu);
        const double cost = rounds * (kp + 2 * D3P_GKB);
        if (cost < best_cost) { best_cost = cost; best = sp; }
    }
    return best;
}

__global__ void k_gemm_reduce(GemmArgs g, int splits)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)g.M * g.N) return;
    const int row = (int)(t / g.N), col = (int)(t % g.N);
    // (all tiles requested at once, like k_vae_finalize: a loop over a run-time count is one memory round trip per tile)
    float tv[D3P_WPART_SPLITS];
#pragma unroll
    for (int z = 0; z < D3P_WPART_SPLITS; ++z) tv[z] = z < splits ? g.part[(size_t)z * g.M * g.N + t] : 0.f;
    float s = 0.f;
#pragma unroll
    for (int z = 0; z < D3P_WPART_SPLITS; ++z) s += z < splits ? tv[z] : 0.f;  // fixed order
    gemm_store(g, row, col, s, g.bias ? g.bias[col + (col >= g.n_seg ? g.bias_njump : 0ll)] : 0.f);
}

int gemm_route(const float* A, long long a_sm, long long a_sk, const float* B, long long b_sk, long long b_sn, int M, int N, int K, int a_last_one,
               const GemmJumps* jumps)
{
    // 16-byte fetches along the unit-stride dimension when every such load is aligned: base pointer, the other stride and the
    // K range of a split (k_per is a multiple of 16) -- the kernels guard the M / N edges themselves, K must be a multiple of 4
    auto aligned16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
    const bool b_plain = !(jumps && (jumps->b_njump || jumps->b_kjump));  // displaced B segments: scalar fetch only
    const bool va = aligned16(A) && K % 4 == 0 && ((a_sk == 1 && a_sm % 4 == 0) || (a_sm == 1 && a_sk % 4 == 0));
    const bool vb = aligned16(B) && K % 4 == 0 && ((b_sn == 1 && b_sk % 4 == 0) || (b_sk == 1 && b_sn % 4 == 0)) && b_plain;
    // 128 x 64 tiles (k_gemm_f32_w8): whole float4s only (see its header)
    // (also for a short, very deep product -- the V1 weight gradient, 51 x 400 x 4096: its workgroups run alone on their CUs, where
    // the 64 x 64 kernel's one-slice pipeline leaves every load latency exposed: 21.7 us)
    const int m_real_h = a_last_one ? M - 1 : M, K4 = (K + 3) & ~3;
    // (the eight-wave kernel takes any K: a k-fast operand needs a row stride of at least roundup4(K))
    const bool va8 = aligned16(A) && ((a_sk == 1 && a_sm % 4 == 0 && a_sm >= K4) || (a_sm == 1 && a_sk % 4 == 0 && a_sk >= ((m_real_h + 3) & ~3)));
    const bool vb8 = aligned16(B) && ((b_sn == 1 && b_sk % 4 == 0 && N % 4 == 0) || (b_sk == 1 && b_sn % 4 == 0 && b_sn >= K4)) && b_plain;
    const bool big = va8 && vb8 && (M > 96 || (M > 32 && K >= 2048));
    static const bool fp32_mfma = getenv("D3P_GEMM_FP32_MFMA") != nullptr;  // developer switch: the fp32-MFMA kernel for the large products
    if (big) return fp32_mfma ? GEMM_ROUTE_W8 : GEMM_ROUTE_BF16X3;
    return GEMM_ROUTE_F32 | (va ? GEMM_ROUTE_F32_VA : 0) | (vb ? GEMM_ROUTE_F32_VB : 0);
}

// part / part_floats: optional split-K scratch.  At B = 4096 the GEMMs of this model are parallelism-starved on 256 CUs (bigger
// tiles lose), so besides the weight gradients the two N = 400 forward / backward-data GEMMs are split too.
// The split count is chosen so that short grids (the weight-gradient
// GEMMs: K = batch, M x N = a weight matrix) still put a few workgroups on every CU.
int gemm(hipStream_t s, const float* A, long long a_sm, long long a_sk, const float* B, long long b_sk, long long b_sn, float* C, int ldc, int M, int N,
         int K, const float* bias, float alpha, int accumulate, const GemmOpts& o)
{
    static const GemmJumps no_jumps = {0x7fffffff, 0x7fffffff, 0, 0, 0, 0};
    const GemmJumps& j = o.jumps ? *o.jumps : no_jumps;
    GemmArgs g;
    g.A = A; g.B = B; g.C = C; g.bias = bias;
    g.M = M; g.N = N; g.K = K;
    g.a_sm = a_sm; g.a_sk = a_sk; g.b_sk = b_sk; g.b_sn = b_sn;
    g.ldc = ldc; g.alpha = alpha; g.accumulate = accumulate;
    g.a_last_one = o.a_last_one; g.epi = o.epi; g.C2 = o.C2;
    g.a_exact16 = o.a_exact16; g.a_exact_nonce = o.a_exact_nonce; g.b_row_scale = o.b_row_scale;
    g.ep_x = o.ep_x; g.ep_ll = o.ep_ll; g.ep_xx = o.ep_xx;
    g.ex_zu = o.ex_zu; g.ex_eps = o.ex_eps; g.ex_Z = o.ex_Z; g.ex_sc = o.ex_sc;
    g.n_seg = j.n_seg; g.k_seg = j.k_seg;
    g.b_njump = j.b_njump; g.b_kjump = j.b_kjump; g.bias_njump = j.bias_njump; g.c_njump = j.c_njump;
    const int route = gemm_route(A, a_sm, a_sk, B, b_sk, b_sn, M, N, K, o.a_last_one, o.jumps);
    const bool bf16 = route == GEMM_ROUTE_BF16X3, big = bf16 || route == GEMM_ROUTE_W8;   // big: the eight-wave kernels' 128 x 64 tiles
    const bool ak = a_sk == 1, bn = b_sn == 1;
    if (o.b_row_scale && !(bf16 && bn)) return fail(D3P_E_INVALID_ARG, "gemm: b_row_scale on a product that does not take the bf16 kernel");
    if (o.epi == 4 && !(bf16 && !o.part && ak && bn && o.ep_x && o.ep_ll && o.ep_xx))
        return fail(D3P_E_INVALID_ARG, "gemm: epilogue 4 on a product that does not take the bf16 kernel unsplit");
    const int tm = big ? D3P_GTM : D3P_GT;
    const unsigned tiles = cdiv(N, D3P_GT) * cdiv(M, tm);
    int splits = 1;
    if (o.part && tiles < (big ? 160u : 512u) && K >= 8 * D3P_GK) {
        splits = big ? (bf16 ? gemm_group_splits(tiles, K) : (int)(512 / tiles))   // (fp32 kernel: two 8-wave workgroups per CU, one round)
                     : (int)((1024 + tiles - 1) / tiles);
        const int max_by_k = K / (4 * D3P_GK);
        if (splits > max_by_k && !bf16) splits = max_by_k;   // (gemm_group_splits keeps its K ranges at two slices or more)
        if (splits > 16) splits = 16;  // the reduction adds the partial tiles serially
        const size_t max_by_mem = o.part_floats / ((size_t)M * N);
        if ((size_t)splits > max_by_mem) splits = (int)max_by_mem;
        if (splits < 1) splits = 1;
    }
    if (o.force_splits > 0 && o.part && big) {
        splits = o.force_splits;
        const size_t max_by_mem = o.part_floats / ((size_t)M * N);
        if ((size_t)splits > max_by_mem) splits = (int)max_by_mem;
        if (splits < 1) splits = 1;
    }
    const int kq = big ? D3P_GKB : D3P_GK;  // K slice of the kernel: a split starts on a slice boundary
    int k_per = (K + splits - 1) / splits;
    k_per = (k_per + kq - 1) / kq * kq;
    splits = (K + k_per - 1) / k_per;
    g.k_per = k_per;
    g.part = splits > 1 ? o.part : nullptr;
    const dim3 grid(cdiv(N, D3P_GT), cdiv(M, tm), splits);
    GemmGroupPlan* const group = o.group;
    const bool joins = bf16 && group && o.splits_left && group->n < D3P_GROUP_MAX && (group->n == 0 || (group->ak == ak && group->bn == bn));
    if (o.report) {
        o.report->route = joins ? GEMM_ROUTE_GROUPED : route;
        o.report->splits = splits;
    }
    if (o.plan_only) return D3P_OK;
    if (joins) {
        const int p = group->n++;
        group->ak = ak;
        group->bn = bn;
        group->q.g[p] = g;
        group->q.gx[p] = grid.x;
        group->q.gy[p] = grid.y;
        group->q.cnt[p] = grid.x * grid.y * grid.z;
        *o.splits_left = splits > 1 ? splits : 0;
        return D3P_OK;
    }
    if (o.epi == 4) hipLaunchKernelGGL((k_gemm_bf16x3<true, true, true>), grid, dim3(512), 0, s, g);
    else if (bf16) D3P_LAUNCH_XY(k_gemm_bf16x3, ak, bn, grid, dim3(512), s, g);
    else if (big) D3P_LAUNCH_XY(k_gemm_f32_w8, ak, bn, grid, dim3(512), s, g);
    else D3P_LAUNCH_XY(k_gemm_f32, route & GEMM_ROUTE_F32_VA, route & GEMM_ROUTE_F32_VB, grid, dim3(256), s, g);
    if (o.splits_left) *o.splits_left = splits > 1 ? splits : 0;
    if (splits > 1 && !o.splits_left) hipLaunchKernelGGL(k_gemm_reduce, dim3(cdiv((uint64_t)M * N, 256)), dim3(256), 0, s, g, splits);
    return check_launch("k_gemm_f32");
}

}  // namespace d3p

using namespace d3p;

extern "C" {

// C = alpha op(A) op(B) (+ bias) (+ C) on the matrix cores; exported so the GEMM can be tested on its own.
int d3p_gemm_f32(void* stream, const float* A_dev, int64_t a_sm, int64_t a_sk, const float* B_dev, int64_t b_sk, int64_t b_sn,
                 float* C_dev, int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias_dev, float alpha, int32_t accumulate)
{
    D3P_REQUIRE(A_dev && B_dev && C_dev, "d3p_gemm_f32: null pointer");
    D3P_REQUIRE(M >= 1 && N >= 1 && K >= 1 && ldc >= N, "d3p_gemm_f32: bad shape");
    return gemm((hipStream_t)stream, A_dev, a_sm, a_sk, B_dev, b_sk, b_sn, C_dev, ldc, M, N, K, bias_dev, alpha, accumulate);
}

// ---- test aids: gemm() with its options, and the grouped launch, reachable on their own.  Production never calls them.
// Everything gemm() cannot run, or a product of the VAE step never asks for, is refused before anything is enqueued.
static int gemm_ex_check(const float* A, int64_t a_sm, int64_t a_sk, const float* B, const float* C, int32_t ldc, int32_t M, int32_t N,
                         int32_t K, int32_t accumulate, const d3p_gemm_opts* o, int force_splits)
{
    D3P_REQUIRE(A && B && C && o, "d3p_gemm_f32_ex: null pointer");
    D3P_REQUIRE(M >= 1 && N >= 1 && K >= 1 && ldc >= N, "d3p_gemm_f32_ex: bad shape");
    D3P_REQUIRE(!o->a_last_one || M >= 2, "d3p_gemm_f32_ex: a_last_one needs a row of A in memory");
    D3P_REQUIRE(o->epi >= 0 && o->epi <= 4, "d3p_gemm_f32_ex: unknown epilogue");
    D3P_REQUIRE(!(o->epi == 1 || o->epi == 2) || o->C2, "d3p_gemm_f32_ex: epilogues 1 and 2 need C2");
    D3P_REQUIRE(o->epi != 3 || (o->ex_zu && o->ex_eps && o->ex_Z == N && ldc >= 2 * N), "d3p_gemm_f32_ex: epilogue 3 needs ex_zu, ex_eps, ex_Z = N and ldc >= 2 N");
    D3P_REQUIRE(o->epi != 4 || (o->ep_x && o->ep_ll && o->ep_xx && !accumulate && !o->has_jumps && !o->leave_split),
                "d3p_gemm_f32_ex: epilogue 4 needs ep_x, ep_ll, ep_xx and a plain product");
    D3P_REQUIRE(!o->leave_split || o->epi == 0, "d3p_gemm_f32_ex: tiles are left unreduced by products without an epilogue only");
    D3P_REQUIRE(!o->part || o->part_floats >= (uint64_t)M * N, "d3p_gemm_f32_ex: part_floats is smaller than M N");
    D3P_REQUIRE(o->part || o->part_floats == 0, "d3p_gemm_f32_ex: part_floats without part");
    if (force_splits != 0) {
        D3P_REQUIRE(o->part, "d3p_gemm_f32_ex: force_splits without part");
        D3P_REQUIRE(gemm_split_count_ok(force_splits, K), "d3p_gemm_f32_ex: a force_splits that gemm_group_splits cannot return for this K");
        D3P_REQUIRE(o->part_floats >= (uint64_t)force_splits * M * N, "d3p_gemm_f32_ex: part_floats is smaller than force_splits M N");
    }
    if (o->exact16_word) {
        const int64_t m_real = o->a_last_one ? M - 1 : M;
        const bool contiguous = (a_sk == 1 && a_sm == K) || (a_sm == 1 && a_sk == m_real);
        D3P_REQUIRE(contiguous && (reinterpret_cast<uintptr_t>(A) & 15u) == 0 && (m_real * K) % 4 == 0,
                    "d3p_gemm_f32_ex: the exactness pass needs a contiguous, 16-byte aligned A of a multiple of 4 elements");
    }
    return D3P_OK;
}

static void gemm_ex_opts(const d3p_gemm_opts* o, GemmOpts& g, GemmJumps& j, int* left, GemmReport* rep)
{
    g.a_last_one = o->a_last_one;
    g.part = o->part; g.part_floats = (size_t)o->part_floats;
    g.epi = o->epi; g.C2 = o->C2; g.ex_zu = o->ex_zu; g.ex_eps = o->ex_eps; g.ex_Z = o->ex_Z; g.ex_sc = o->ex_sc;
    g.ep_x = o->ep_x; g.ep_ll = o->ep_ll; g.ep_xx = o->ep_xx;
    if (o->has_jumps) {
        j.n_seg = o->n_seg; j.k_seg = o->k_seg;
        j.b_njump = o->b_njump; j.b_kjump = o->b_kjump; j.bias_njump = o->bias_njump; j.c_njump = o->c_njump;
        g.jumps = &j;
    }
    g.b_row_scale = o->b_row_scale;
    g.force_splits = o->force_splits;
    g.splits_left = o->leave_split ? left : nullptr;
    g.a_exact16 = o->exact16_word; g.a_exact_nonce = o->exact16_nonce;
    g.report = rep;
}

// the exactness pass over A, as vae_enqueue_forward enqueues it in front of the products that read the flag
static void gemm_ex_flag(hipStream_t s, const float* A, int32_t M, int32_t K, const d3p_gemm_opts* o)
{
    exact16_flag_launch(s, A, (size_t)(o->a_last_one ? M - 1 : M) * K / 4, o->exact16_word, o->exact16_nonce);
}

int d3p_gemm_f32_ex(void* stream, const float* A_dev, int64_t a_sm, int64_t a_sk, const float* B_dev, int64_t b_sk, int64_t b_sn,
                    float* C_dev, int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias_dev, float alpha, int32_t accumulate,
                    const d3p_gemm_opts* opts, d3p_gemm_report* report)
{
    D3P_REQUIRE(report, "d3p_gemm_f32_ex: null report");
    if (int rc = gemm_ex_check(A_dev, a_sm, a_sk, B_dev, C_dev, ldc, M, N, K, accumulate, opts, opts ? opts->force_splits : 0)) return rc;
    GemmOpts g;
    GemmJumps j;
    GemmReport rep = {0, 0};
    int left = 0;
    gemm_ex_opts(opts, g, j, &left, &rep);
    g.plan_only = true;   // gemm()'s own refusals, before the exactness pass is enqueued
    if (int rc = gemm((hipStream_t)stream, A_dev, a_sm, a_sk, B_dev, b_sk, b_sn, C_dev, ldc, M, N, K, bias_dev, alpha, accumulate, g)) return rc;
    g.plan_only = false;
    if (opts->exact16_word) gemm_ex_flag((hipStream_t)stream, A_dev, M, K, opts);
    const int rc = gemm((hipStream_t)stream, A_dev, a_sm, a_sk, B_dev, b_sk, b_sn, C_dev, ldc, M, N, K, bias_dev, alpha, accumulate, g);
    report->route = rep.route;
    report->splits = rep.splits;
    report->splits_left = left;
    return rc;
}

int d3p_gemm_f32_group(void* stream, d3p_gemm_member* members, int32_t n, int32_t force_splits, const float* sum_in_dev, float* sum_out_dev,
                       uint32_t sum_n)
{
    D3P_REQUIRE(members && n >= 1 && n <= D3P_GROUP_MAX + 1, "d3p_gemm_f32_group: 1 .. D3P_GROUP_MAX + 1 members");
    D3P_REQUIRE((sum_in_dev != nullptr) == (sum_out_dev != nullptr) && (sum_in_dev || sum_n == 0), "d3p_gemm_f32_group: sum_in and sum_out come together");
    hipStream_t s = (hipStream_t)stream;
    for (int p = 0; p < n; ++p) {   // every refusal before the first launch
        d3p_gemm_member& m = members[p];
        D3P_REQUIRE(m.opts.leave_split && m.opts.force_splits == 0 && m.opts.epi == 0, "d3p_gemm_f32_group: members leave their tiles and take the group's force_splits");
        if (int rc = gemm_ex_check(m.A, m.a_sm, m.a_sk, m.B, m.C, m.ldc, m.M, m.N, m.K, m.accumulate, &m.opts, force_splits)) return rc;
        GemmOpts g;
        GemmJumps j;
        GemmReport rep = {0, 0};
        int left = 0;
        gemm_ex_opts(&m.opts, g, j, &left, &rep);
        g.force_splits = force_splits;
        g.plan_only = true;
        if (int rc = gemm(s, m.A, m.a_sm, m.a_sk, m.B, m.b_sk, m.b_sn, m.C, m.ldc, m.M, m.N, m.K, m.bias, m.alpha, m.accumulate, g)) return rc;
    }
    GemmGroupPlan plan;
    GemmJumps jumps[D3P_GROUP_MAX + 1];
    for (int p = 0; p < n; ++p) {
        d3p_gemm_member& m = members[p];
        GemmOpts g;
        GemmReport rep = {0, 0};
        int left = 0;
        gemm_ex_opts(&m.opts, g, jumps[p], &left, &rep);
        g.force_splits = force_splits;
        g.group = &plan;
        if (m.opts.exact16_word) gemm_ex_flag(s, m.A, m.M, m.K, &m.opts);
        if (int rc = gemm(s, m.A, m.a_sm, m.a_sk, m.B, m.b_sk, m.b_sn, m.C, m.ldc, m.M, m.N, m.K, m.bias, m.alpha, m.accumulate, g)) return rc;
        m.report.route = rep.route;
        m.report.splits = rep.splits;
        m.report.splits_left = left;
        m.joined = rep.route == GEMM_ROUTE_GROUPED ? 1 : 0;
    }
    if (plan.n > 0) { plan.sum_in = sum_in_dev; plan.sum_out = sum_out_dev; plan.sum_n = sum_n; }
    else D3P_REQUIRE(!sum_in_dev, "d3p_gemm_f32_group: no member joined the group, so nothing sums sum_in");
    return gemm_group_launch(s, plan);
}

}  // extern "C"
