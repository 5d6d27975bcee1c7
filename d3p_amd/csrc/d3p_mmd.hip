// Gaussian-kernel row sums of two tables (d3p_amd/mmd.py, include/d3p_hip.h): per row of the first table and per
// bandwidth of a ladder the float64 sum of k(a_i, b_j) over the rows of the second -- what the maximum mean discrepancy (Gretton et al.
// 2012) and its witness function reduce -- from a Gram walk on the matrix cores.  The entry d3p_kernel_sums with its host checks, its
// three kernels, the query functions of its geometry, workspace and bound, and the test aid that forces the segment count.
//
// THE RULE.  a[i * a_ld + c] is row i < na of the first table in column c < d, b[j * b_ld + c] row j < nb of the second, both float32
// (dtype 0) or both int32 (dtype 1: converted to float32 when loaded, exact for |v| <= 2^24, which is what the Python layer admits).
// shift and scale are d float32 each, or null (a null pointer skips that step):
//     t_c     = fl32(fl32(x_c - shift_c) * scale_c)                      (one IEEE subtraction, one IEEE multiplication, never fused)
//     r_i     = the float32 chain r <- fmaf(t_c, t_c, r) over c = 0 .. d-1 ascending, from +0     (k_mmd_norms: a thread per row)
//     g_ij    = sum_c ta_ic tb_jc                                         (v_mfma_f32_32x32x2_f32, float32 accumulator: THE ORDER)
//     q_ij    = fmaf(-2, g_ij, fl32(ra_i + rb_j)), and 0 where that is < 0  (a select, not fmaxf: a NaN stays a NaN)
//     k_ij^0  = exp2(fl32(-gamma0 * q_ij))                                (the native v_exp_f32)
//     k_ij^b  = fl32(k_ij^(b-1) * k_ij^(b-1)),  b = 1 .. B-1              (bandwidth b has the exponent coefficient gamma0 2^b)
//     out[b * na + i] = sum over the admissible j of k_ij^b              in float64, in THE ORDER below
// for B = 1 .. 8 bandwidths and one finite gamma0 > 0: one transcendental and B - 1 multiplications a pair.  The ADMISSIBLE j of row i
// are pair_admissible's (d3p_pair_tile.h): all j < nb, without j == i when exclude_diagonal is set (which requires na == nb).  A row
// without an admissible j gets 0.  A NaN or +-inf element in row i of a makes out[b][i] NaN for every b and touches no other row; one
// anywhere in b makes every row NaN: flags of the loaded words, taken while the tables are staged, never from the arithmetic.  Finite
// elements whose t, r, g or q overflows follow IEEE from there (q = +inf gives k = 0; inf - inf a NaN in that row).
//
// THE ORDER, which is ONE order.
//   * g_ij: the columns are cut into CHUNKS of 32 and a chunk into 16 PAIRS (2 p, 2 p + 1); g starts at +0 in an accumulator register,
//     the chunks are taken ascending, within a chunk the pairs ascending, and pair p is ONE instruction acc <- acc + ta_2p tb_2p + ta_2p+1
//     tb_2p+1 (as d3p_project_rows states it: how the instruction orders its two products is not documented, and the bound holds for any
//     order).  The padding is t = 0: dp = 2 ceil(d / 2) columns meet where the operands of a stay in registers, 32 ceil(d / 32) otherwise;
//     a zero product changes no bit of a sum, so g does not depend on which.
//   * the rows of b are cut into TILES of 32, the tiles into nseg SEGMENTS of tps consecutive tiles (d3p_kernel_sums_segments,
//     _segment_tiles), a segment into GROUPS of G = 64 consecutive tiles from its first (d3p_kernel_sums_group_tiles).
//   * a float32 PARTIAL per (row i, lane s = j mod 32, bandwidth) adds k_ij^b over the tiles of a group in ascending order onto +0 (a
//     pair that is not admissible adds +0): at most G additions.
//   * at a group's end the 32 partials of a row are widened to float64 (exact) and added: s = 0 .. 15 ascending onto +0, s = 16 .. 31
//     ascending onto +0, then the first sum plus the second.  The groups of a segment are added in ascending order onto +0; the
//     segments in ascending order onto +0 by the merge launch.  Strips of a never meet: a row belongs to one.
// G is derived, not chosen: a float32 chain of m additions of non-negative terms errs by at most gamma_(m-1) of its sum, and the
// smallest Gram term the rule can have -- one chunk, dp = 32 -- already costs k a relative 2 gamma_32 ~ 64 u; the chain is allowed the
// same 64 u, so m - 1 <= 64 and, a tile adding one term to a partial, G = 64 tiles.
//
// DETERMINISM.  Repeated calls with equal arguments and an equal forced segment count give equal bits.  out[b][i] depends on row i's
// values, the table b, nb, d, the dtype, shift, scale, gamma0, the flag (with it: i) and on the segment geometry (nseg, tps), which the
// host derives from (na, nb) ALONE -- so through it on na, and on nothing else of a: not on the other rows of a, a_ld, b_ld, the
// alignment of either table (the 16-byte and the word loads stage equal bits), the row's place in its strip, B (rung b is the same for
// every B > b) or what the workspace held.  The three walks of d3p_amd.mmd on EQUAL tables do not give equal bits where it matters: the
// (x, y) walk holds the diagonal's k_ii = exp2(-gamma0 q_ii) with q_ii the clamped rounding residue of ra + ra - 2 g_ii, the excluded
// walks add the exact 1 on the host; mmd2 of equal tables is within the bound of 0, not 0.
//
// THE KERNELS.  k_mmd_norms: a thread per row of a and of b writes r to the workspace (O((na + nb) d), beside an O(na nb d) walk).
// k_mmd_walk<B, RES>: a workgroup of four wavefronts owns a STRIP of 128 rows of a, 32 per wavefront, and one segment of b.
//   * The tile of b (32 rows) is staged ONCE per workgroup in LDS and shared by the four wavefronts: conversion, shift, scale and the
//     zeroing of dead rows and columns (a select AFTER the arithmetic) on the way in, the non-finite flags from the loaded words.  With
//     a row pitch of KW + 1 words the operand read bs[s][2 p + h] of a half-wave hits 32 distinct banks.  16-byte loads where the
//     table's address and ld allow them (16-byte aligned, ld a multiple of 4), one word per thread otherwise; the lanes that share a
//     row are the smallest power of two that covers the columns, so d = 2 costs one load a thread, not sixteen.
//   * The tile is DOUBLE-BUFFERED: the next tile's global loads are issued before the current tile's products and held in registers,
//     its LDS stores go to the other buffer, and ONE barrier a tile orders them (a buffer is written two barriers after it was read).
//   * RES (d <= 64, d3p_kernel_sums_resident_cols): the wavefront's A operands -- one float per lane and column pair -- are loaded
//     once, ceil(d / 2) <= 32 VGPRs, and stay for the whole walk; the tile of b holds all d columns.  The limit is the register
//     report's (tools/kernel_resources.py): at 32 operand registers the instances B <= 5 fit the 256 registers that let two workgroups
//     share a CU (174 .. 246 VGPRs; their launch bounds ask for it), and the second workgroup is what overlaps one's epilogue with the
//     other's matrix instructions; 64 operand registers (d <= 128) leave that to B = 1 alone.  B = 6 .. 8 take 280 .. 326 registers
//     and one workgroup a CU: 16 partials a bandwidth cannot be had for less.
//   * else: the strip of a (128 x 32) and the tile of b (32 x 32) stream through LDS in chunks of 32 columns, both double-buffered the
//     same way; the accumulators stay in registers across the chunks.
//   * The epilogue runs on the 16 accumulator registers: lane (h, s) holds the rows 8 (v / 4) + 4 h + v % 4 of column s of the tile.
//     It adds ra (16 registers, loaded once) and rb (one load a tile, issued a tile ahead), clamps, takes ONE exp2, squares B - 1
//     times and adds into 16 x B float32 partials.  At a group's end the partials pass through 32 x 33 floats of the wavefront's own
//     LDS to the row's two lanes (order above); lane r < 32 keeps row r's B float64 totals.
//   * STATIC LDS only (GramLds, d3p_gram_tile.h): RES 16640 + 8 + 16896 + 516 = 34060 bytes; streaming 8448 + 33792 + 16896 + 516 = 59652 bytes.  The streaming
//     form takes 328 .. 454 registers (the compiler keeps the 20 row addresses of both load forms and a chunk's 32 operands ahead):
//     one workgroup a CU, no scratch; a cap at 256 spills, so there is none.  Open gain: the load form as a template argument.
// k_mmd_merge: a thread per row adds the segments' cells in ascending order and writes NaN where a flag is set.
// THE GRID.  The strips of a alone do not fill the chip below ~10^5 rows, so the host cuts b into nseg = min(tiles of b, ceil(1024 /
// strips)) segments (1024 workgroups: 256 CUs x 2 resident x 2), tps = ceil(tiles / nseg) tiles each, from (na, nb) alone.  Workspace:
// 8 B nseg na bytes of cells (b, segment, row), 4 nseg na of flag words, 4 (na + nb) of norms; nseg na <= 2^17 + na + 127 under the
// rule, so the cells stay below 8 B (2^17 + na + 127) bytes.  Every word read is written earlier in the same call.  No atomics, no
// scratch, no host synchronisation, no allocation, no dynamic LDS; nothing outside out and the workspace is written.
//
// THE BOUND, against the float64 k of the same float32 t (q formed by differences), u = 2^-24, gamma_m = m u / (1 - m u), dp = 32 ceil(d
// / 32) (the larger padding), with ra, rb, q the exact values of the float32 t and A_ij = sum_c |ta_ic| |tb_jc| <= sqrt(ra rb):
//     dq_ij = gamma_(dp+2) (ra_i + rb_j) + 2 gamma_dp A_ij + u (q_ij + that) + (2 dp + 4) 2^-126
//             (the norm chains and the addition; Higham's dot product bound for any order, rounded or fused products; the fmaf; flushed
//             subnormals.  The clamp moves q^ towards q >= 0 and costs nothing.)
//     E_0   = 2^(gamma0 (dq + u (q + dq))) (1 + 2 u) - 1      (k(q + dq) = k(q) 2^(-gamma0 dq); the rounding of -gamma0 q^; v_exp_f32 is
//             accurate to 1 ulp <= 2 u relative: "V_EXP_F32 ... 1 ULP accuracy", AMD Instinct CDNA3/CDNA4 ISA guide, VOP1 table)
//     E_b   = (1 + E_(b-1))^2 (1 + u) - 1                      (the ladder doubles the relative error a rung and rounds once)
//     |k^_ij^b - k_ij^b| <= E_b k_ij^b + 2^-125                (a result below 2^-126 may be flushed to 0, on any rung)
//     |out^[b][i] - out[b][i]| <= (1 + gamma_63) sum_j (E_b k_ij^b + 2^-125) + (gamma_63 + gamma64_R) sum_j k^_ij^b
// where gamma_63 is the float32 chain of a group and R = d3p_kernel_sums_roundings(na, nb) = 16 + 1 + ceil(tps / 64) + nseg float64
// additions lie on a row (gamma64 with u = 2^-53).  On tables centred on load with gamma0 ~ 1 / median q this is a few dp u of k.
#include "d3p_device.h"
#include "d3p_host.h"
#include "d3p_pair_tile.h"
#include "d3p_gram_tile.h"   // the staging, the load forms, the product loop and the segment rule: shared with d3p_sinkhorn.hip

#define D3P_MM_GROUP 64u                              // G: tiles of b a float32 partial adds before it is widened
#define D3P_MM_MAX_B 8u

static int32_t g_mm_segments = 0;   // d3p_kernel_sums_set_segments: 0 = the rule

namespace d3p {

struct MmArgs {
    const uint32_t* a; const uint32_t* b; int32_t dtype; int64_t a_ld, b_ld; uint32_t na, nb, d, excl, nseg, tps, B, vec_a, vec_b;
    const float* shift; const float* scale; float gamma0;
    float* ra; float* rb; double* cell; uint32_t* flag;   // the workspace
    double* out;
};

// THE EPILOGUE of gram_walk: the partials of a group and the float64 totals of the segment
template <int NB>
struct MmEpilogue {
    float part[NB][16];
    double tot[NB];
    float ngamma;
    uint32_t nb, excl;

    __device__ __forceinline__ MmEpilogue(const MmArgs& a) : ngamma(-a.gamma0), nb(a.nb), excl(a.excl)
    {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            tot[b] = 0.0;
#pragma unroll
            for (int v = 0; v < 16; ++v) part[b][v] = 0.0f;
        }
    }
    __device__ __forceinline__ void ahead(uint32_t, bool) {}
    __device__ __forceinline__ void advance() {}
    __device__ __forceinline__ bool bad() const { return false; }

    // the tile's 16 x 32 pairs of lane (half, sub): q, the clamp, ONE exp2, the ladder, the partials; a group's end
    __device__ __forceinline__ void tile(const gram_f16v& acc, const float (&ra)[16], float rb, uint32_t r0, uint32_t half, uint32_t j, uint32_t k,
                                         bool last, float* red, uint32_t lane)
    {
#pragma clang fp contract(off)
#pragma unroll
        for (uint32_t v = 0; v < 16u; ++v) {
            const uint32_t i = r0 + gram_acc_row(v, half);
            const float s = ra[v] + rb;
            float q = __fmaf_rn(-2.0f, acc[v], s);
            q = q < 0.0f ? 0.0f : q;                               // (a NaN compares false and stays)
            float kv = __builtin_amdgcn_exp2f(ngamma * q);
            kv = pair_admissible(i, j, nb, excl) ? kv : 0.0f;      // (0 squared is 0: masked once for every rung)
            part[0][v] = part[0][v] + kv;
#pragma unroll
            for (int b = 1; b < NB; ++b) {
                kv = kv * kv;
                part[b][v] = part[b][v] + kv;
            }
        }
        if ((k + 1u) % D3P_MM_GROUP == 0u || last) flush(red, lane);
    }

    // a group's end: the partials, widened, to the rows' float64 totals (lanes r and r + 32 hold row r's; THE ORDER) and back to +0
    __device__ __forceinline__ void flush(float* red, uint32_t lane)
    {
#pragma clang fp contract(off)
        const uint32_t half = lane >> 5, sub = lane & 31u;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (uint32_t v = 0; v < 16u; ++v) {
                red[gram_acc_row(v, half) * D3P_GRAM_RED + sub] = part[b][v];
                part[b][v] = 0.0f;
            }
            pair_wave_sync();
            double s = 0.0;
#pragma unroll
            for (uint32_t e = 0; e < 16u; ++e) s = s + (double)red[sub * D3P_GRAM_RED + 16u * half + e];
            const double o = __shfl_xor(s, 32, 64);
            tot[b] = tot[b] + (s + o);                             // (a + b is commutative: both lanes end with equal bits)
            pair_wave_sync();
        }
    }
};

__global__ __launch_bounds__(256) void k_mmd_norms(MmArgs a) { gram_norms(a); }

template <int NB, bool RES>
__global__ __launch_bounds__(64 * D3P_GRAM_WAVES, (RES && NB <= 5) ? 2 : 1) void k_mmd_walk(MmArgs a)
{
    __shared__ GramLds<RES> lds;
    MmEpilogue<NB> epi(a);
    const uint32_t flags = gram_walk<RES>(a, lds, epi);
    const uint32_t lane = threadIdx.x & 63u, seg = pair_split_segment(a.nseg);
    const uint32_t row = pair_split_tile(a.nseg) * D3P_GRAM_STRIP + (threadIdx.x >> 6) * D3P_GRAM_TILE + lane;
    if (lane < D3P_GRAM_TILE && row < a.na) {
#pragma unroll
        for (int b = 0; b < NB; ++b) a.cell[(uint64_t)b * a.nseg * a.na + pair_cell(seg, a.na, row)] = epi.tot[b];
        a.flag[pair_cell(seg, a.na, row)] = flags;
    }
}

// the second launch: one thread per row adds its cells in ascending segment order
__global__ __launch_bounds__(256) void k_mmd_merge(MmArgs a)
{
#pragma clang fp contract(off)
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.na) return;
    uint32_t flags = 0u;
    for (uint32_t seg = 0; seg < a.nseg; ++seg) flags |= a.flag[pair_cell(seg, a.na, i)];
    for (uint32_t b = 0; b < a.B; ++b) {
        double total = 0.0;
        for (uint32_t seg = 0; seg < a.nseg; ++seg) total = total + a.cell[(uint64_t)b * a.nseg * a.na + pair_cell(seg, a.na, i)];
        a.out[(uint64_t)b * a.na + i] = flags ? (double)__builtin_nanf("") : total;
    }
}

static size_t mm_workspace(uint32_t na, uint32_t nb, uint32_t B)
{
    if (!gram_sizes_ok(na, nb) || B < 1 || B > D3P_MM_MAX_B) return 0;
    const size_t cells = (size_t)gram_segments(na, nb, g_mm_segments) * na;   // < 2^26 x 2^31
    return cells * 8u * B + cells * 4u + ((size_t)na + nb) * 4u;
}

template <int NB>
static int mm_launch(const char* what, bool res, unsigned groups, hipStream_t stream, const MmArgs& a)
{
    if (res) return pair_launch_merged(what, k_mmd_walk<NB, true>, k_mmd_merge, groups, a.na, stream, a);
    return pair_launch_merged(what, k_mmd_walk<NB, false>, k_mmd_merge, groups, a.na, stream, a);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_kernel_sums_strip_rows(void) { return D3P_GRAM_STRIP; }

uint32_t d3p_kernel_sums_group_tiles(void) { return D3P_MM_GROUP; }

uint32_t d3p_kernel_sums_resident_cols(void) { return D3P_GRAM_RES; }

uint32_t d3p_kernel_sums_max_bandwidths(void) { return D3P_MM_MAX_B; }

uint32_t d3p_kernel_sums_segments(uint32_t na, uint32_t nb) { return gram_segments(na, nb, g_mm_segments); }

uint32_t d3p_kernel_sums_segment_tiles(uint32_t na, uint32_t nb) { return gram_sizes_ok(na, nb) ? gram_segment_tiles(na, nb, g_mm_segments) : 0u; }

uint32_t d3p_kernel_sums_roundings(uint32_t na, uint32_t nb)
{
    if (!gram_sizes_ok(na, nb)) return 0u;
    // a half row's sixteen; the halves; the groups of a segment; the segments
    return 16u + 1u + (gram_segment_tiles(na, nb, g_mm_segments) + D3P_MM_GROUP - 1u) / D3P_MM_GROUP + gram_segments(na, nb, g_mm_segments);
}

size_t d3p_kernel_sums_workspace(uint32_t na, uint32_t nb, uint32_t n_bandwidths) { return mm_workspace(na, nb, n_bandwidths); }

int d3p_kernel_sums_set_segments(int32_t segments)
{
    if (segments < 0) return fail(D3P_E_INVALID_ARG, "d3p_kernel_sums_set_segments: segments must be 0 (the rule) or a count >= 1, got %d", segments);
    g_mm_segments = segments;
    return D3P_OK;
}

int d3p_kernel_sums(void* stream, const void* a_dev, const void* b_dev, int32_t dtype, int64_t a_ld, int64_t b_ld, uint32_t na, uint32_t nb,
                    uint32_t d, const float* shift_dev, const float* scale_dev, float gamma0, uint32_t n_bandwidths, int32_t exclude_diagonal,
                    double* out_dev, void* ws_dev, size_t ws_bytes)
{
    const char* what = "d3p_kernel_sums";
    if (!a_dev || !b_dev || !out_dev || !ws_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)a_dev | (uintptr_t)b_dev | (uintptr_t)shift_dev | (uintptr_t)scale_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if ((((uintptr_t)out_dev | (uintptr_t)ws_dev) & 7u) != 0) return fail(D3P_E_INVALID_ARG, "%s: out_dev or ws_dev is not aligned to 8 bytes", what);
    if (const int rc = pair_check_pair(what, dtype, a_ld, b_ld, na, nb, d)) return rc;
    if (const int rc = pair_check_diagonal(what, exclude_diagonal, na, nb)) return rc;
    if (n_bandwidths < 1 || n_bandwidths > D3P_MM_MAX_B)
        return fail(D3P_E_INVALID_ARG, "%s: n_bandwidths must be in 1 .. %u, got %u", what, D3P_MM_MAX_B, n_bandwidths);
    if (!(gamma0 > 0.0f) || !std::isfinite(gamma0)) return fail(D3P_E_INVALID_ARG, "%s: gamma0 must be finite and > 0", what);
    MmArgs a;
    const unsigned groups = gram_prepare(what, g_mm_segments, a_dev, b_dev, dtype, a_ld, b_ld, na, nb, d, shift_dev, scale_dev, a);
    if (!groups) return D3P_E_UNSUPPORTED;
    const size_t need = mm_workspace(na, nb, n_bandwidths);
    if (ws_bytes < need) return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_bytes, need);
    if (!is_device_ptr(a_dev) || !is_device_ptr(b_dev) || !is_device_ptr(out_dev) || !is_device_ptr(ws_dev) || (shift_dev && !is_device_ptr(shift_dev)) ||
        (scale_dev && !is_device_ptr(scale_dev)))
        return fail(D3P_E_INVALID_ARG, "%s: the tables, the shift, the scale, the output and the workspace must be device memory", what);
    a.excl = (uint32_t)exclude_diagonal; a.B = n_bandwidths; a.gamma0 = gamma0; a.out = out_dev;
    const size_t cells = (size_t)a.nseg * na;
    char* ws = static_cast<char*>(ws_dev);
    a.cell = reinterpret_cast<double*>(ws);
    a.flag = reinterpret_cast<uint32_t*>(ws + cells * 8u * n_bandwidths);
    a.ra = reinterpret_cast<float*>(ws + cells * 8u * n_bandwidths + cells * 4u);
    a.rb = a.ra + na;
    if (const int rc = gram_launch_norms(what, k_mmd_norms, (hipStream_t)stream, a)) return rc;
    const bool res = d <= D3P_GRAM_RES;
    switch (n_bandwidths) {
        case 1: return mm_launch<1>(what, res, groups, (hipStream_t)stream, a);
        case 2: return mm_launch<2>(what, res, groups, (hipStream_t)stream, a);
        case 3: return mm_launch<3>(what, res, groups, (hipStream_t)stream, a);
        case 4: return mm_launch<4>(what, res, groups, (hipStream_t)stream, a);
        case 5: return mm_launch<5>(what, res, groups, (hipStream_t)stream, a);
        case 6: return mm_launch<6>(what, res, groups, (hipStream_t)stream, a);
        case 7: return mm_launch<7>(what, res, groups, (hipStream_t)stream, a);
        default: return mm_launch<8>(what, res, groups, (hipStream_t)stream, a);
    }
}

}  // extern "C"
