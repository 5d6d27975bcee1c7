// Soft-min rows of two tables (d3p_amd/sinkhorn.py, include/d3p_hip.h): per row of the first table the base-2
// log-sum-exp of a potential minus the scaled squared distance over the rows of the second -- the one primitive of entropic optimal
// transport in the log domain (Sinkhorn; the debiased divergence of Feydy et al. 2019) -- from d3p_mmd.hip's Gram walk with an ONLINE
// epilogue: a running integer reference and a rescaled sum per row, as an attention kernel keeps them, and never the n_a x n_b matrix.
// The entry d3p_softmin_rows with its host checks, its three kernels, the query functions of its geometry, workspace and bound, and the
// test aid that forces the segment count.
//
// THE RULE.  a, b, dtype, a_ld, b_ld, na, nb, d, shift and scale are d3p_kernel_sums' (d3p_mmd.hip), and so are
//     t_c   = fl32(fl32(x_c - shift_c) * scale_c)                        (one IEEE subtraction, one IEEE multiplication, never fused)
//     r_i   = the float32 chain r <- fmaf(t_c, t_c, r) over c = 0 .. d-1 ascending, from +0     (k_sk_norms: gram_norms)
//     g_ij  = sum_c ta_ic tb_jc                                           (v_mfma_f32_32x32x2_f32, float32 accumulator, d3p_mmd.hip's order)
//     q_ij  = fmaf(-2, g_ij, fl32(ra_i + rb_j)), and 0 where that is < 0   (a select, not fmaxf)
// With one finite gamma > 0, h (nb float32, base-2 units), optional prev (na float64), omega (a double in (0, 1]) and optional logw (na
// float32):
//     v_ij    = fmaf(-gamma, q_ij, h_j)                                   float32
//     L_i     = log2 sum_j 2^(v_ij)          over all j < nb              float64, in THE ORDER below
//     pot_i   = -L_i                          if prev is null
//             = prev_i + omega * ((-L_i) - prev_i)   otherwise            float64, these three operations, never fused
//     out_h_i = fl32(pot_i + logw_i)          if logw and out_h are given (one float64 addition, one conversion)
// pot (float64, na) is always written.  out_h is the h of the opposite walk: a Sinkhorn half-step is one call.  h_j = -inf is a row of
// zero weight and adds nothing; if every h_j is -inf, L_i = -inf and (prev null) pot_i = +inf, no NaN.  A NaN or +inf in h makes every
// row NaN; a NaN or +-inf element in row i of a makes row i NaN (pot and out_h) and touches no other; one anywhere in b every row: flags
// of the loaded words, taken while the tables and h are staged, never from the arithmetic.  A finite v below -2^127 counts as -inf.
//
// THE ORDER, which is ONE order.  g_ij, the tiles of 32 rows of b, the nseg segments of tps consecutive tiles (d3p_softmin_rows_segments,
// _segment_tiles: d3p_kernel_sums' rule, from (na, nb) alone) and the GROUPS of G = 64 consecutive tiles of a segment
// (d3p_softmin_rows_group_tiles) are d3p_mmd.hip's.
//   * a float32 PAIR (m, s) per (row i, lane s = j mod 32) runs over the tiles of a group in ascending order from (F, +0), F = -2^127
//     the finite FLOOR: m is INTEGER-valued, the floor of the largest v the pair has met (or F), s = sum 2^(v - m).  A tile:
//         m' = max(m, floor(v))      s <- ldexp(s, max(m - m', -300)) + exp2(fl32(v - m'))      m <- m'
//     The rescale is by an exact power of two (v_ldexp_f32; below 2^-300 of an s < 2^7: to 0), so it rounds nothing: s carries the
//     roundings of its at most G additions, of v - m' and of v_exp_f32 alone.  v - m' is ONE rounding: exact by Sterbenz where m' / 2
//     <= v <= 2 m', else at most u |v - m'| absolute -- below 2^-17 of a bit at the 126 bits beyond which the term is flushed anyway.
//     v < m' + 1 always, so a term is < 2 and s < 2 G.
//     m' = m exactly when no floor(v) exceeds its m: then ldexp(s, 0) = s and m' = m change no bit, and a wavefront SKIPS the rescale
//     of a tile under one ballot of that test; the taken and the skipped path give equal bits, and a row's bits do not depend on what
//     the other rows of its wavefront made the ballot say.  F makes m - m', v - m' and the test well defined for v = -inf (m' = m, the
//     term exp2(-inf) = +0) without a select: no NaN is born of (-inf) - (-inf).
//   * at a group's end the 32 pairs of a row pass through the wavefront's own LDS to the row's two lanes, 16 each (s = 0 .. 15, s = 16
//     .. 31): Mh = max of the sixteen m; Sh = sum over s ascending onto +0 of the float64 ldexp(s_s, max(m_s - Mh, -1100)) (exact: a
//     float32 scaled by a power of two, or 0 below 2^-1100); the halves: M2 = max(Mh0, Mh1), S2 = ldexp(Sh0, .) + ldexp(Sh1, .) scaled
//     to M2; the groups of a segment ascending onto (F, +0): M' = max(M, M2), S <- ldexp(S, M - M') + ldexp(S2, M2 - M').  The
//     segments likewise, ascending, by the merge launch, which takes L = M + log2(S) in float64 (S = 0: -inf) and the pot step.
// G is derived as d3p_mmd.hip derives its 64: a float32 chain of m additions of non-negative terms errs by gamma_(m-1) of its sum.
// The smallest Gram term (one chunk, dp = 32) costs q an absolute 2 gamma_32 (ra + rb) ~ 64 u (ra + rb), a term 2^v the relative ln 2
// gamma 64 u (ra + rb); where the walk is worth its name -- epsilon at most half the typical squared distance, gamma = 1 / (2 epsilon
// ln 2), so ln 2 gamma (ra + rb) >= 1 -- that is at least 64 u, the chain is allowed the same, m - 1 <= 64, and G = 64 tiles.
//
// DETERMINISM.  Repeated calls with equal arguments and an equal forced segment count give equal bits.  pot_i depends on row i's values,
// the table b, h, nb, d, the dtype, shift, scale, gamma, prev_i, omega and the segment geometry (from (na, nb) alone); not on the other
// rows of a, a_ld, b_ld, the alignment of either table (the 16-byte and the word loads stage equal bits) or what the workspace held.  A
// row of b with h_j = -inf adds +0 to one s and raises no m: at the tail of the last tile it is as if it were not there.
//
// THE KERNELS.  k_sk_norms: gram_norms.  k_sk_walk<RES>: gram_walk (d3p_gram_tile.h: the strip of 128 rows per workgroup of four
// wavefronts; the tile of b staged once per workgroup, double-buffered with one barrier a tile, pitch KW + 1; 16-byte loads where
// address and ld allow; the operands of a resident in registers up to d = 64 = d3p_softmin_rows_resident_cols(), both tables streaming
// through LDS in 32-column chunks above) with THIS epilogue on the 16 accumulator registers: h_j rides with rb_j, one more load a tile,
// issued a tile ahead, and its flag is taken from that word.  Per pair: the addition and the fmaf of q, the clamp, the fmaf of v, a
// floor and a compare for the ballot, a subtraction, ONE v_exp_f32 and an addition; 32 VGPRs of (m, s) where d3p_kernel_sums holds 16 B
// partials.  The group's end uses the 32 x 33 floats of the wavefront's LDS twice, for m and for s.  STATIC LDS only, gram_walk's.  The
// resident walk takes 178 VGPRs (tools/kernel_resources.py; docs/experiments_sinkhorn.md) and its launch bounds ask for two workgroups
// a CU; the streaming walk one, as d3p_kernel_sums'.  k_sk_merge: a thread per row.
// THE GRID.  d3p_kernel_sums': nseg = min(tiles of b, ceil(1024 / strips)).  Workspace (d3p_softmin_rows_workspace): per (segment, row
// of a) a float64 M, a float64 S and a flag word, 20 bytes; 4 (na + nb) of norms.  Every word read is written earlier in the same
// call.  No atomics, no scratch, no host synchronisation, no allocation, no dynamic LDS; nothing outside pot, out_h and the workspace is
// written.
//
// THE BOUND, in BITS of L, against the float64 log-sum-exp of the same float32 t and h with q by differences; u = 2^-24, dq_ij
// d3p_mmd.hip's, p_ij = 2^(v_ij - L_i) the row's soft-max weights:
//     dv_ij = gamma dq_ij + u (|h_j| + gamma (q_ij + dq_ij)) + u (|v_ij - m| <= 127 where the term is kept) + log2(1 + 2 u)
//             (v moves by gamma dq; the fmaf rounds once, at most u |v|; the subtraction of the reference; v_exp_f32's 1 ulp)
//     |dL_i| <= log2(sum_j p_ij 2^(dv_ij)) + log2(1 + E_sum) + log2(1 + nb 2^-126) + u64 (4 + 2 |L_i|)
//     E_sum  = gamma_64 + gamma64_R,   R = d3p_softmin_rows_roundings(na, nb) = 16 + 1 + ceil(tps / 64) + nseg float64 additions on a row
//             (a far row's large dv counts by its negligible weight; the float32 chain of a group; a term below 2^(m - 126) is flushed,
//             and the row's largest term is >= 1 against its own m; log2 and the addition of M in float64)
// and the pot step adds its three float64 roundings, u64 (|L| + 2 |prev|), out_h the conversion's u |pot + logw|.  On tables centred on
// load, with epsilon a share of the median q, this is a few d u gamma (ra + rb) bits.
#include "d3p_device.h"
#include "d3p_host.h"
#include "d3p_pair_tile.h"
#include "d3p_gram_tile.h"

#define D3P_SK_GROUP 64u            // G: tiles of b a float32 pair runs over before it is merged in float64
#define D3P_SK_FLOOR (-0x1p127f)    // F: the finite floor of every reference

static int32_t g_sk_segments = 0;   // d3p_softmin_rows_set_segments: 0 = the rule

namespace d3p {

struct SkArgs {
    const uint32_t* a; const uint32_t* b; int32_t dtype; int64_t a_ld, b_ld; uint32_t na, nb, d, nseg, tps, vec_a, vec_b;
    const float* shift; const float* scale; float gamma;
    const float* h; const double* prev; double omega; const float* logw;
    float* ra; float* rb; double* cell_m; double* cell_s; uint32_t* flag;   // the workspace
    double* pot; float* out_h;
};

// x 2^(from - to), from <= to: exact, or 0 below 2^-1100 (a NaN difference, born of a flagged row alone, scales to 0 as well)
__device__ __forceinline__ double sk_scale(double x, double from, double to) { return ldexp(x, (int)fmax(from - to, -1100.0)); }

// (M, S) <- (M, S) merged with (m2, s2) by exact scaling to the larger reference
__device__ __forceinline__ void sk_merge(double& M, double& S, double m2, double s2)
{
#pragma clang fp contract(off)
    const double mn = fmax(M, m2);
    S = sk_scale(S, M, mn) + sk_scale(s2, m2, mn);
    M = mn;
}

// THE EPILOGUE of gram_walk: the float32 pairs of a group and the float64 pair of the segment
struct SkEpilogue {
    float m[16], s[16];
    double M, S;
    float ngamma, h_cur, h_next;
    const float* h;
    bool badh;

    __device__ __forceinline__ SkEpilogue(const SkArgs& a) : M((double)D3P_SK_FLOOR), S(0.0), ngamma(-a.gamma), h_cur(0.0f), h_next(0.0f), h(a.h), badh(false)
    {
#pragma unroll
        for (int v = 0; v < 16; ++v) { m[v] = D3P_SK_FLOOR; s[v] = 0.0f; }
    }
    // h_j rides with rb_j; a column beyond nb has no weight; the flag of NaN and +inf from the loaded word
    __device__ __forceinline__ void ahead(uint32_t j, bool live)
    {
        const float w = live ? h[j] : -__builtin_inff();
        badh |= !(w < __builtin_inff());
        h_next = w;
    }
    __device__ __forceinline__ void advance() { h_cur = h_next; }
    __device__ __forceinline__ bool bad() const { return badh; }

    __device__ __forceinline__ void tile(const gram_f16v& acc, const float (&ra)[16], float rb, uint32_t, uint32_t, uint32_t, uint32_t k, bool last,
                                         float* red, uint32_t lane)
    {
#pragma clang fp contract(off)
        float vv[16];
        bool raise = false;
#pragma unroll
        for (uint32_t v = 0; v < 16u; ++v) {
            const float sum = ra[v] + rb;
            float q = __fmaf_rn(-2.0f, acc[v], sum);
            q = q < 0.0f ? 0.0f : q;                               // (a NaN compares false and stays)
            vv[v] = __fmaf_rn(ngamma, q, h_cur);
            raise |= __builtin_floorf(vv[v]) > m[v];
        }
        if (__builtin_amdgcn_ballot_w64(raise) != 0ull) {           // (wave-uniform; where no lane raises, every ldexp would be by 2^0)
#pragma unroll
            for (uint32_t v = 0; v < 16u; ++v) {
                const float mn = fmaxf(m[v], __builtin_floorf(vv[v]));
                s[v] = __builtin_ldexpf(s[v], (int)fmaxf(m[v] - mn, -300.0f));
                m[v] = mn;
            }
        }
#pragma unroll
        for (uint32_t v = 0; v < 16u; ++v) s[v] = s[v] + __builtin_amdgcn_exp2f(vv[v] - m[v]);
        if ((k + 1u) % D3P_SK_GROUP == 0u || last) flush(red, lane);
    }

    // a group's end: the pairs to the row's float64 pair (lanes r and r + 32 hold row r's; THE ORDER) and back to (F, +0)
    __device__ __forceinline__ void flush(float* red, uint32_t lane)
    {
#pragma clang fp contract(off)
        const uint32_t half = lane >> 5, sub = lane & 31u;
        float me[16];
#pragma unroll
        for (uint32_t v = 0; v < 16u; ++v) {
            red[gram_acc_row(v, half) * D3P_GRAM_RED + sub] = m[v];
            m[v] = D3P_SK_FLOOR;
        }
        pair_wave_sync();
#pragma unroll
        for (uint32_t e = 0; e < 16u; ++e) me[e] = red[sub * D3P_GRAM_RED + 16u * half + e];
        pair_wave_sync();
#pragma unroll
        for (uint32_t v = 0; v < 16u; ++v) {
            red[gram_acc_row(v, half) * D3P_GRAM_RED + sub] = s[v];
            s[v] = 0.0f;
        }
        pair_wave_sync();
        float mh = me[0];
#pragma unroll
        for (uint32_t e = 1; e < 16u; ++e) mh = fmaxf(mh, me[e]);
        double sh = 0.0;
#pragma unroll
        for (uint32_t e = 0; e < 16u; ++e) sh = sh + sk_scale((double)red[sub * D3P_GRAM_RED + 16u * half + e], (double)me[e], (double)mh);
        pair_wave_sync();
        const float mo = __shfl_xor(mh, 32, 64);
        const double so = __shfl_xor(sh, 32, 64);
        const double m2 = (double)fmaxf(mh, mo);
        const double s2 = sk_scale(sh, (double)mh, m2) + sk_scale(so, (double)mo, m2);   // (a + b is commutative: both lanes end with equal bits)
        sk_merge(M, S, m2, s2);
    }
};

__global__ __launch_bounds__(256) void k_sk_norms(SkArgs a) { gram_norms(a); }

template <bool RES>
__global__ __launch_bounds__(64 * D3P_GRAM_WAVES, RES ? 2 : 1) void k_sk_walk(SkArgs a)
{
    __shared__ GramLds<RES> lds;
    SkEpilogue epi(a);
    const uint32_t flags = gram_walk<RES>(a, lds, epi);
    const uint32_t lane = threadIdx.x & 63u, seg = pair_split_segment(a.nseg);
    const uint32_t row = pair_split_tile(a.nseg) * D3P_GRAM_STRIP + (threadIdx.x >> 6) * D3P_GRAM_TILE + lane;
    if (lane < D3P_GRAM_TILE && row < a.na) {
        a.cell_m[pair_cell(seg, a.na, row)] = epi.M;
        a.cell_s[pair_cell(seg, a.na, row)] = epi.S;
        a.flag[pair_cell(seg, a.na, row)] = flags;
    }
}

// the second launch: one thread per row merges its cells in ascending segment order, takes L and the pot step
__global__ __launch_bounds__(256) void k_sk_merge(SkArgs a)
{
#pragma clang fp contract(off)
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.na) return;
    uint32_t flags = 0u;
    double M = (double)D3P_SK_FLOOR, S = 0.0;
    for (uint32_t seg = 0; seg < a.nseg; ++seg) {
        flags |= a.flag[pair_cell(seg, a.na, i)];
        sk_merge(M, S, a.cell_m[pair_cell(seg, a.na, i)], a.cell_s[pair_cell(seg, a.na, i)]);
    }
    const double L = M + log2(S);                                  // (S = 0: -inf)
    double pot = -L;
    if (a.prev) {
        const double p = a.prev[i], diff = pot - p, step = a.omega * diff;
        pot = p + step;
    }
    if (flags) pot = (double)__builtin_nanf("");
    a.pot[i] = pot;
    if (a.logw && a.out_h) a.out_h[i] = (float)(pot + (double)a.logw[i]);
}

static size_t sk_workspace(uint32_t na, uint32_t nb)
{
    if (!gram_sizes_ok(na, nb)) return 0;
    const size_t cells = (size_t)gram_segments(na, nb, g_sk_segments) * na;   // < 2^26 x 2^31
    return cells * 20u + ((size_t)na + nb) * 4u;
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_softmin_rows_group_tiles(void) { return D3P_SK_GROUP; }

uint32_t d3p_softmin_rows_resident_cols(void) { return D3P_GRAM_RES; }

uint32_t d3p_softmin_rows_segments(uint32_t na, uint32_t nb) { return gram_segments(na, nb, g_sk_segments); }

uint32_t d3p_softmin_rows_segment_tiles(uint32_t na, uint32_t nb) { return gram_sizes_ok(na, nb) ? gram_segment_tiles(na, nb, g_sk_segments) : 0u; }

uint32_t d3p_softmin_rows_roundings(uint32_t na, uint32_t nb)
{
    if (!gram_sizes_ok(na, nb)) return 0u;
    // a half row's sixteen; the halves; the groups of a segment; the segments
    return 16u + 1u + (gram_segment_tiles(na, nb, g_sk_segments) + D3P_SK_GROUP - 1u) / D3P_SK_GROUP + gram_segments(na, nb, g_sk_segments);
}

size_t d3p_softmin_rows_workspace(uint32_t na, uint32_t nb) { return sk_workspace(na, nb); }

int d3p_softmin_rows_set_segments(int32_t segments)
{
    if (segments < 0) return fail(D3P_E_INVALID_ARG, "d3p_softmin_rows_set_segments: segments must be 0 (the rule) or a count >= 1, got %d", segments);
    g_sk_segments = segments;
    return D3P_OK;
}

int d3p_softmin_rows(void* stream, const void* a_dev, const void* b_dev, int32_t dtype, int64_t a_ld, int64_t b_ld, uint32_t na, uint32_t nb,
                     uint32_t d, const float* shift_dev, const float* scale_dev, float gamma, const float* h_dev, const double* prev_dev, double omega,
                     const float* logw_dev, double* pot_dev, float* out_h_dev, void* ws_dev, size_t ws_bytes)
{
    const char* what = "d3p_softmin_rows";
    if (!a_dev || !b_dev || !h_dev || !pot_dev || !ws_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)a_dev | (uintptr_t)b_dev | (uintptr_t)shift_dev | (uintptr_t)scale_dev | (uintptr_t)h_dev | (uintptr_t)logw_dev | (uintptr_t)out_h_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if ((((uintptr_t)pot_dev | (uintptr_t)prev_dev | (uintptr_t)ws_dev) & 7u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: pot_dev, prev_dev or ws_dev is not aligned to 8 bytes", what);
    if (const int rc = pair_check_pair(what, dtype, a_ld, b_ld, na, nb, d)) return rc;
    if (!(gamma > 0.0f) || !std::isfinite(gamma)) return fail(D3P_E_INVALID_ARG, "%s: gamma must be finite and > 0", what);
    if (!(omega > 0.0 && omega <= 1.0)) return fail(D3P_E_INVALID_ARG, "%s: omega must be in (0, 1]", what);
    if ((logw_dev == nullptr) != (out_h_dev == nullptr)) return fail(D3P_E_INVALID_ARG, "%s: logw_dev and out_h_dev are given together or not at all", what);
    SkArgs a;
    const unsigned groups = gram_prepare(what, g_sk_segments, a_dev, b_dev, dtype, a_ld, b_ld, na, nb, d, shift_dev, scale_dev, a);
    if (!groups) return D3P_E_UNSUPPORTED;
    const size_t need = sk_workspace(na, nb);
    if (ws_bytes < need) return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_bytes, need);
    if (!is_device_ptr(a_dev) || !is_device_ptr(b_dev) || !is_device_ptr(h_dev) || !is_device_ptr(pot_dev) || !is_device_ptr(ws_dev) ||
        (shift_dev && !is_device_ptr(shift_dev)) || (scale_dev && !is_device_ptr(scale_dev)) || (prev_dev && !is_device_ptr(prev_dev)) ||
        (logw_dev && !is_device_ptr(logw_dev)) || (out_h_dev && !is_device_ptr(out_h_dev)))
        return fail(D3P_E_INVALID_ARG, "%s: the tables, the vectors, the outputs and the workspace must be device memory", what);
    a.gamma = gamma; a.h = h_dev; a.prev = prev_dev; a.omega = omega; a.logw = logw_dev; a.pot = pot_dev; a.out_h = out_h_dev;
    const size_t cells = (size_t)a.nseg * na;
    char* ws = static_cast<char*>(ws_dev);
    a.cell_m = reinterpret_cast<double*>(ws);
    a.cell_s = a.cell_m + cells;
    a.flag = reinterpret_cast<uint32_t*>(ws + cells * 16u);
    a.ra = reinterpret_cast<float*>(ws + cells * 20u);
    a.rb = a.ra + na;
    if (const int rc = gram_launch_norms(what, k_sk_norms, (hipStream_t)stream, a)) return rc;
    if (d <= D3P_GRAM_RES) return pair_launch_merged(what, k_sk_walk<true>, k_sk_merge, groups, na, (hipStream_t)stream, a);
    return pair_launch_merged(what, k_sk_walk<false>, k_sk_merge, groups, na, (hipStream_t)stream, a);
}

}  // extern "C"
