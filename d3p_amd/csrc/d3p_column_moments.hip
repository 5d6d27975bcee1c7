// Column means and the centred cross-product matrix of a table (d3p_amd/covariance.py, include/d3p_hip.h): what the
// covariance, the Pearson correlation and the Gaussian Frechet distance of a synthetic table against the real one are made of, as ONE
// contraction over the ROWS on the matrix cores -- never a float32 Gram product of the raw values (which cancels), never a float64 copy
// of the table.  The entry d3p_column_moments with its host checks, its four kernels and the query functions of their geometry.
//
// THE RULE is the shifted-data algorithm (per row: d3p_shifted_sums.h).  x[i * ld + c] is row i < n in column c < d, float32 (dtype 0)
// or int32 (dtype 1: converted to float32 when loaded, exact for |v| <= 2^24, which is what the Python layer admits).
//     S_c  = sum_i (double)x_ic  in the order below      c_c = (float)(S_c / n), the SHIFT      flag_c = "S_c is not finite"
//     t_ic = fl32(x_ic - c_c)                            (one float32 subtraction, in registers)
//     G_ce = sum_i t_ic t_ie                             (v_mfma_f32_32x32x2_f32 in strips, the strips in float64: THE ORDER)
//     s_c  = sum_i (double)t_ic                          (float64 throughout)
//     mean_c = (double)c_c + s_c / n                     m2_ce = G_ce - s_c s_e / n
// s_c is of the order of n times the rounding of c_c, so the subtrahend is tiny and nothing cancels.  (c, e) and (e, c) are written
// from the one value computed for c <= e.  A FLAGGED column (a NaN, a +inf or a -inf in it: a float64 sum of finite float32 values
// cannot overflow, so the flag is exactly that) gets mean = NaN and NaN in its whole row and column of m2, from the flag and never
// from inf - inf; its shift is 0.  It touches no other column: an entry of G is made of its two columns alone.  Finite values whose
// t or products overflow float32 follow IEEE from there.
//
// THE ORDER, which is ONE order (there is one form).  With L = 64 (d3p_column_moments_strip_rows), R = d3p_column_moments_segment_rows
// (n, d), a multiple of 4 L, and the rows cut into SEGMENTS of R.  EVERY MERGE OVER SEGMENTS adds them in 8 CHUNKS of ceil(segments / 8)
// consecutive segments, each chunk in ascending order onto 0, then the chunks in ascending order onto 0 (cm_chunk, cm_meet).
//   * S_c (its own segments: R of one block pair, d3p_column_moments_segment_rows(n, 1)): thread (phase p = 0 .. 3) of a segment adds
//     the rows p + 4 k into four accumulators k mod 4, each in ascending k onto 0, then (a0 + a1) + (a2 + a3); the phases in ascending
//     p onto 0; the segments merged as above.
//   * G_ce, s_c: the columns are cut into BLOCKS of 64 (two TILES of 32); a workgroup owns a block pair P <= Q and a segment, and each of
//     its four wavefronts ONE tile pair (P's tile ta) x (Q's tile tb) and every row pair of the segment (rows 2 j, 2 j + 1), in
//     ascending j, in float32 accumulators of the matrix instruction (whose internal order over its two rows is not documented); after
//     every L / 2 row pairs (a STRIP: L rows) and at the end the accumulators are widened and added onto float64 registers, which
//     started at 0.  s_c: per row parity in float64, ascending j onto 0; then even + odd.  The segments merged as above.
// The longest float64 chain of G is A = R / L + ceil(segments / 8) + 8 additions, of s it is R / 2 + 1 + ceil(segments / 8) + 8.
// Rows >= n and columns >= d are zeroed by select AFTER the subtraction; their lanes read a word INSIDE the table instead (the
// segment's last row, column 0), so that no load sits behind a branch.
//
// THE KERNEL (k_cm_products).  Lane l of a wavefront supplies A row / B column l % 32 at k = l / 32 of the matrix instruction: for
// both operands that is column c0 + l % 32 of table row r0 + l / 32, so a half-wave reads 128 contiguous bytes of one row and the
// wavefront feeds the matrix pipe straight from global memory: no LDS on the way in.  Per row pair: two dwords per lane (one on a
// diagonal tile pair, whose B operand is its A register), the subtraction, the select, ONE matrix instruction and two float64 additions
// for s.  On a diagonal block pair the wavefront of the mirror tile pair leaves at once: 3 tile pairs, not 4.  A tile of the table is
// loaded by the two wavefronts that use it (the second from the CU's cache).  Row pairs are taken in groups of 8 and the next group's
// loads are issued before the current group's products.  The wavefront holds 16 float32 accumulators and 16 float64 partials: 116
// VGPRs, four wavefronts per SIMD, which is what hides the loads' latency.  The instruction takes 16 passes of 4 cycles = 64 cycles, so
// a strip is 32 x 64 = 2048 matrix cycles and its flush (16 conversions + 16 float64 additions of 4 cycles) 128: 6.25 %.
// No LDS in k_cm_products; the merges use 256 to 8192 bytes.  No atomics, no scratch, no dynamic LDS, no host synchronisation, no
// allocation.  Every word of the workspace that is read is written before in the same call.
//
// DETERMINISM.  Repeated calls give equal bits.  m2[c][e] depends on columns c and e, n, d and the dtype alone: not on ld, m2_ld, the
// other columns' contents or what the workspace held before.
#include "d3p_device.h"
#include "d3p_host.h"

#define D3P_CM_T 2u             // tiles of 32 columns along a side of a block
#define D3P_CM_BLOCK (32u * D3P_CM_T)             // columns of a block (d3p_column_moments_block_cols)
#define D3P_CM_WAVES (D3P_CM_T * D3P_CM_T)        // one wavefront per tile pair of the block pair
#define D3P_CM_STRIP 64u        // L: rows a wavefront contracts in float32 between two flushes (d3p_column_moments_strip_rows)
#define D3P_CM_GROUP 8u         // row pairs of a wavefront in flight
#define D3P_CM_SUMCOLS 64u      // columns of a workgroup of the column-sum kernel
#define D3P_CM_MIN_SEG 1024u    // the shortest segment
#define D3P_CM_CHUNKS 8u        // the segments' partials are added in this many chunks of consecutive segments
#define D3P_CM_TARGET 1024u     // workgroups aimed at when d is small
#define D3P_CM_G (D3P_CM_BLOCK * D3P_CM_BLOCK)    // float64 words of a partial: the products of the block pair ...
#define D3P_CM_PART (D3P_CM_G + 2u * D3P_CM_BLOCK)   // ... and s of the pair's columns

namespace d3p {

typedef float cm_f16v __attribute__((ext_vector_type(16)));

struct CmArgs {
    const uint32_t* x; int32_t dtype; int64_t ld; uint32_t n, d, nb, nseg, R, sum_nseg, sum_R; uint64_t npairs;
    float* shift; uint32_t* flag; double* colsum; double* sums; double* parts;   // the workspace: [dpad] | [dpad] | [sum_nseg][dpad] | [npairs][2 B] | [npairs][nseg][PART]
    double* mean; double* m2; int64_t m2_ld;
};

__device__ __forceinline__ float cm_value(int32_t dtype, uint32_t w) { return dtype ? (float)(int32_t)w : __uint_as_float(w); }

// launch A, first half: the float64 column sums of one segment of 64 columns
__global__ __launch_bounds__(256) void k_cm_colsum(CmArgs a)
{
    __shared__ double part[4][D3P_CM_SUMCOLS];
    const uint32_t lane = threadIdx.x & 63u, phase = threadIdx.x >> 6;
    const uint32_t col = blockIdx.x * D3P_CM_SUMCOLS + lane, seg = blockIdx.y;
    const uint64_t lo = (uint64_t)seg * a.sum_R, hi = lo + a.sum_R < a.n ? lo + a.sum_R : a.n;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (col < a.d) {
        const uint32_t* p = a.x + col;
        uint64_t r = lo + phase;
        for (; r + 12u < hi; r += 16u) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += (double)cm_value(a.dtype, p[(int64_t)(r + 4u * k) * a.ld]);
        }
        for (int k = 0; r < hi; r += 4u, ++k) acc[k] += (double)cm_value(a.dtype, p[(int64_t)r * a.ld]);
    }
    part[phase][lane] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    __syncthreads();
    if (phase == 0) {
        double s = 0.0;
        for (uint32_t w = 0; w < 4u; ++w) s += part[w][lane];
        a.colsum[(size_t)seg * ((size_t)a.nb * D3P_CM_BLOCK) + col] = s;
    }
}

// The sum of nseg float64 words p[k stride] in THE ORDER of every merge over segments: chunk c of D3P_CM_CHUNKS holds the
// ceil(nseg / 8) consecutive segments from c ceil(nseg / 8), added in ascending order onto 0 (eight loads in flight); the caller adds
// the chunks in ascending order onto 0
__device__ __forceinline__ double cm_chunk(const double* p, size_t stride, uint32_t nseg, uint32_t c)
{
    const uint32_t len = (nseg + D3P_CM_CHUNKS - 1u) / D3P_CM_CHUNKS, lo = c * len;
    if (lo >= nseg) return 0.0;
    const uint32_t hi = lo + len < nseg ? lo + len : nseg;
    double s = 0.0;
    uint32_t k = lo;
    for (; k + 8u <= hi; k += 8u) {
        double v[8];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) v[u] = p[(size_t)(k + u) * stride];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) s += v[u];
    }
    for (; k < hi; ++k) s += p[(size_t)k * stride];
    return s;
}

// the chunks of `items` (<= 128) words met in LDS: thread (item, chunk) has `mine`; returns the sum for chunk 0's threads
template <uint32_t ITEMS>
__device__ __forceinline__ double cm_meet(double (&part)[D3P_CM_CHUNKS][ITEMS], uint32_t item, uint32_t chunk, double mine)
{
    part[chunk][item] = mine;
    __syncthreads();
    double s = 0.0;
    if (chunk == 0)
        for (uint32_t c = 0; c < D3P_CM_CHUNKS; ++c) s += part[c][item];
    return s;
}

// launch A, second half: the segments' sums merged, the shift and the flag; 32 columns x 8 chunks per workgroup
__global__ __launch_bounds__(256) void k_cm_shift(CmArgs a)
{
    __shared__ double part[D3P_CM_CHUNKS][32];
    const size_t dpad = (size_t)a.nb * D3P_CM_BLOCK;
    const uint32_t item = threadIdx.x & 31u, chunk = threadIdx.x >> 5;
    const size_t col = (size_t)blockIdx.x * 32u + item;      // < dpad: a multiple of 32
    const double s = cm_meet<32>(part, item, chunk, cm_chunk(a.colsum + col, dpad, a.sum_nseg, chunk));
    if (chunk != 0) return;
    const bool bad = !(fabs(s) <= 1.7976931348623157e308);
    a.shift[col] = bad ? 0.0f : (float)(s / (double)a.n);
    a.flag[col] = bad ? 1u : 0u;
}

// the block pair P <= Q of index p among nb blocks: row P of the upper triangle starts at P nb - P (P - 1) / 2.  The root gives P
// to within one; the two loops settle it in integers
__device__ __forceinline__ void cm_pair(uint64_t p, uint32_t nb, uint32_t& P, uint32_t& Q)
{
    const double b = 2.0 * (double)nb + 1.0;
    uint64_t row = (uint64_t)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
    if (row >= nb) row = nb - 1u;
    auto start = [nb](uint64_t r) { return r * nb - r * (r - 1u) / 2u; };
    while (row > 0 && start(row) > p) --row;
    while (row + 1u < nb && start(row + 1u) <= p) ++row;
    P = (uint32_t)row;
    Q = (uint32_t)(row + (p - start(row)));
}

// launch B: the products of one block pair over one segment; wavefront (ta, tb) owns the tile pair (P's tile ta) x (Q's tile tb)
__global__ __launch_bounds__(64 * D3P_CM_WAVES) void k_cm_products(CmArgs a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t half = lane >> 5, sub = lane & 31u;
    const uint32_t ta = wave / D3P_CM_T, tb = wave % D3P_CM_T;
    uint32_t P, Q;
    cm_pair(blockIdx.x, a.nb, P, Q);
    const bool diag = P == Q;
    if (diag && ta > tb) return;          // the mirror of tile pair (tb, ta): never read (there is no barrier in this kernel)
    const bool same = diag && ta == tb;   // the B operand is the A register
    const uint32_t seg = blockIdx.y;
    const uint64_t lo = (uint64_t)seg * a.R;
    const uint32_t rows = (uint32_t)(lo + a.R < a.n ? a.R : a.n - lo);
    const uint32_t npair = (rows + 1u) / 2u;      // row pairs of this segment, the last may hold one row
    const uint32_t col_a = P * D3P_CM_BLOCK + ta * 32u + sub, col_b = Q * D3P_CM_BLOCK + tb * 32u + sub;
    const bool live_a = col_a < a.d, live_b = col_b < a.d;
    const float shift_a = live_a ? a.shift[col_a] : 0.0f, shift_b = live_b ? a.shift[col_b] : 0.0f;
    // the lane's columns in the segment's first row; a dead column reads column 0 and is zeroed by the select
    const uint32_t* base_a = a.x + (int64_t)lo * a.ld + (live_a ? col_a : 0u);
    const uint32_t* base_b = a.x + (int64_t)lo * a.ld + (live_b ? col_b : 0u);
    cm_f16v acc;
    double s_a = 0.0, s_b = 0.0;
    double wide[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) { acc[v] = 0.0f; wide[v] = 0.0; }
    // the words of a group of row pairs, without a branch (so that the loads of the next group stay in flight under the products of
    // this one): a row beyond the segment's last reads the last row, a dead column column 0 -- both inside the table, both zeroed by
    // the select after the subtraction
    auto load = [&](uint32_t j0, uint32_t (&wa)[D3P_CM_GROUP], uint32_t (&wb)[D3P_CM_GROUP]) {
#pragma unroll
        for (uint32_t g = 0; g < D3P_CM_GROUP; ++g) {
            const uint32_t r = 2u * (j0 + g) + half;
            const int64_t off = (int64_t)(r < rows ? r : rows - 1u) * a.ld;
            wa[g] = base_a[off];
            if (!same) wb[g] = base_b[off];
        }
    };
    uint32_t cur_a[D3P_CM_GROUP] = {}, cur_b[D3P_CM_GROUP] = {}, nxt_a[D3P_CM_GROUP] = {}, nxt_b[D3P_CM_GROUP] = {};
    uint32_t done = 0;     // row pairs since the last flush
    load(0u, cur_a, cur_b);
    for (uint32_t j0 = 0; j0 < npair; j0 += D3P_CM_GROUP) {
        const uint32_t jn = j0 + D3P_CM_GROUP;
        if (jn < npair) load(jn, nxt_a, nxt_b);
#pragma unroll
        for (uint32_t g = 0; g < D3P_CM_GROUP; ++g) {
            if (j0 + g < npair) {    // (uniform over the wavefront)
                const bool row_live = 2u * (j0 + g) + half < rows;
                const float va = cm_value(a.dtype, cur_a[g]) - shift_a;
                const float t_a = (live_a && row_live) ? va : 0.0f;
                float t_b = t_a;
                if (!same) {
                    const float vb = cm_value(a.dtype, cur_b[g]) - shift_b;
                    t_b = (live_b && row_live) ? vb : 0.0f;
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(t_a, t_b, acc, 0, 0, 0);
                s_a += (double)t_a;
                s_b += (double)t_b;
                ++done;
            }
        }
        if (done >= D3P_CM_STRIP / 2u || jn >= npair) {   // the strip's end (done is a multiple of the group: never beyond L / 2)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                wide[v] += (double)acc[v];
                acc[v] = 0.0f;
            }
            done = 0;
        }
#pragma unroll
        for (uint32_t g = 0; g < D3P_CM_GROUP; ++g) { cur_a[g] = nxt_a[g]; cur_b[g] = nxt_b[g]; }
    }
    // word (tile pair, register v, lane) of the partial at 1024 wave + 64 v + lane
    double* out = a.parts + ((size_t)blockIdx.x * a.nseg + seg) * D3P_CM_PART;
#pragma unroll
    for (int v = 0; v < 16; ++v) out[wave * 1024u + 64u * (uint32_t)v + lane] = wide[v];
    // s of a column: the even rows' half, then the odd rows'.  P's tile ta is written by the wavefront (ta, 0), Q's tile tb by (0, tb);
    // on a diagonal pair (ta, ta) writes both
    const double sum_a = s_a + __shfl_down(s_a, 32), sum_b = s_b + __shfl_down(s_b, 32);
    if (lane < 32u) {
        if (diag ? same : tb == 0u) out[D3P_CM_G + ta * 32u + lane] = sum_a;
        if (diag ? same : ta == 0u) out[D3P_CM_G + D3P_CM_BLOCK + tb * 32u + lane] = sum_b;
    }
}

// launch C, first half: s of the pair's 2 B columns merged over the segments, and the means; 128 words x 8 chunks per workgroup
__global__ __launch_bounds__(1024) void k_cm_sums(CmArgs a)
{
    __shared__ double part[D3P_CM_CHUNKS][2u * D3P_CM_BLOCK];
    uint32_t P, Q;
    cm_pair(blockIdx.x, a.nb, P, Q);
    const uint32_t item = threadIdx.x & (2u * D3P_CM_BLOCK - 1u), chunk = threadIdx.x / (2u * D3P_CM_BLOCK);
    const double* parts = a.parts + (size_t)blockIdx.x * a.nseg * D3P_CM_PART + D3P_CM_G + item;
    const double s = cm_meet<2u * D3P_CM_BLOCK>(part, item, chunk, cm_chunk(parts, D3P_CM_PART, a.nseg, chunk));
    if (chunk != 0) return;
    a.sums[(size_t)blockIdx.x * (2u * D3P_CM_BLOCK) + item] = s;
    const uint32_t c = P * D3P_CM_BLOCK + item;
    if (P == Q && item < D3P_CM_BLOCK && c < a.d) a.mean[c] = a.flag[c] ? (double)__builtin_nanf("") : (double)a.shift[c] + s / (double)a.n;
}

// launch C, second half: the products merged over the segments, m2 and its mirror; blockIdx.y: 32 of the pair's words x 8 chunks
__global__ __launch_bounds__(256) void k_cm_finish(CmArgs a)
{
    __shared__ double part[D3P_CM_CHUNKS][32];
    uint32_t P, Q;
    cm_pair(blockIdx.x, a.nb, P, Q);
    const uint32_t item = threadIdx.x & 31u, chunk = threadIdx.x >> 5;
    const uint32_t at = blockIdx.y * 32u + item;
    const double* parts = a.parts + (size_t)blockIdx.x * a.nseg * D3P_CM_PART + at;
    const uint32_t q = at >> 10, v = (at >> 6) & 15u, lane = at & 63u;
    const bool mirror = P == Q && q / D3P_CM_T > q % D3P_CM_T;    // a tile pair no wavefront wrote: not read (uniform over the workgroup)
    const double g = cm_meet<32>(part, item, chunk, mirror ? 0.0 : cm_chunk(parts, D3P_CM_PART, a.nseg, chunk));
    if (chunk != 0) return;
    const uint32_t i = 8u * (v >> 2) + 4u * (lane >> 5) + (v & 3u), j = lane & 31u;   // the matrix instruction's D[i][j]
    const uint32_t ci = (q / D3P_CM_T) * 32u + i, ej = (q % D3P_CM_T) * 32u + j;       // within the blocks P and Q
    const uint32_t c = P * D3P_CM_BLOCK + ci, e = Q * D3P_CM_BLOCK + ej;
    if (c >= a.d || e >= a.d || c > e) return;     // (c > e: a diagonal pair's lower triangle, the mirror's)
    const double* s = a.sums + (size_t)blockIdx.x * (2u * D3P_CM_BLOCK);
    double m = g - s[ci] * s[D3P_CM_BLOCK + ej] / (double)a.n;
    if (a.flag[c] | a.flag[e]) m = (double)__builtin_nanf("");
    a.m2[(int64_t)c * a.m2_ld + e] = m;
    a.m2[(int64_t)e * a.m2_ld + c] = m;
}

static uint32_t cm_blocks(uint32_t d) { return (uint32_t)(((uint64_t)d + D3P_CM_BLOCK - 1u) / D3P_CM_BLOCK); }

static uint64_t cm_pairs(uint32_t d) { const uint64_t nb = cm_blocks(d); return nb * (nb + 1u) / 2u; }

static bool cm_shape_ok(uint64_t n, uint32_t d) { return n >= 1 && n <= 0xFFFFFFFEull && d >= 1; }

// the rows of a segment: a function of n and d alone.  About D3P_CM_TARGET workgroups over the block pairs, whole strips for every
// wavefront, never below D3P_CM_MIN_SEG; so there are at most D3P_CM_TARGET + 1 segments
static uint32_t cm_rows_for(uint64_t n, uint64_t pairs)
{
    const uint64_t want = pairs >= D3P_CM_TARGET ? 1u : D3P_CM_TARGET / pairs;
    const uint64_t unit = 4u * D3P_CM_STRIP;
    uint64_t R = ((n + want - 1u) / want + unit - 1u) / unit * unit;
    if (R < D3P_CM_MIN_SEG) R = D3P_CM_MIN_SEG;
    if (R > 0xFFFFFF00ull) R = 0xFFFFFF00ull;    // (n beyond 2^32 - 256 in one segment: two, so that R fits 32 bits)
    return (uint32_t)R;
}

static uint32_t cm_segment_rows(uint64_t n, uint32_t d) { return cm_shape_ok(n, d) ? cm_rows_for(n, cm_pairs(d)) : 0u; }

// the rows of a segment of the column sums: as if there were one block pair (about D3P_CM_TARGET workgroups per 64 columns)
static uint32_t cm_sum_rows(uint64_t n) { return cm_rows_for(n, 1u); }

static uint32_t cm_segments(uint64_t n, uint32_t R) { return (uint32_t)((n + R - 1u) / R); }

static size_t cm_workspace(uint64_t n, uint32_t d)
{
    if (!cm_shape_ok(n, d)) return 0;
    const uint32_t R = cm_segment_rows(n, d), nseg = cm_segments(n, R);
    const uint64_t pairs = cm_pairs(d), dpad = (uint64_t)cm_blocks(d) * D3P_CM_BLOCK;
    if (pairs * nseg > 0x7fffffffull) return 0;    // (a grid the entry refuses; also keeps the bytes within 64 bits)
    return (size_t)(dpad * 8u + (uint64_t)cm_segments(n, cm_sum_rows(n)) * dpad * 8u + pairs * 2u * D3P_CM_BLOCK * 8u + pairs * nseg * D3P_CM_PART * 8u);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_column_moments_block_cols(void) { return D3P_CM_BLOCK; }

uint32_t d3p_column_moments_strip_rows(void) { return D3P_CM_STRIP; }

uint32_t d3p_column_moments_segment_rows(uint64_t n, uint32_t d) { return cm_segment_rows(n, d); }

size_t d3p_column_moments_workspace(uint64_t n, uint32_t d) { return cm_workspace(n, d); }

int d3p_column_moments(void* stream, const void* x_dev, int32_t dtype, int64_t ld, uint64_t n, uint32_t d, double* mean_dev, double* m2_dev,
                       int64_t m2_ld, void* ws_dev, size_t ws_bytes)
{
    const char* what = "d3p_column_moments";
    if (!x_dev || !mean_dev || !m2_dev || !ws_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if (((uintptr_t)x_dev & 3u) != 0) return fail(D3P_E_INVALID_ARG, "%s: x_dev is not aligned to 4 bytes", what);
    if ((((uintptr_t)mean_dev | (uintptr_t)m2_dev | (uintptr_t)ws_dev) & 7u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: mean_dev, m2_dev or ws_dev is not aligned to 8 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (n < 1 || n > 0xFFFFFFFEull) return fail(D3P_E_INVALID_ARG, "%s: 1 <= n <= 2^32 - 2 rows are required", what);
    if (d < 1) return fail(D3P_E_INVALID_ARG, "%s: d >= 1 is required", what);
    if (ld < 0 || (uint64_t)ld < d) return fail(D3P_E_INVALID_ARG, "%s: ld >= d is required", what);
    if (n > (uint64_t)INT64_MAX / (uint64_t)ld) return fail(D3P_E_INVALID_ARG, "%s: n * ld does not fit 63 bits", what);
    if (m2_ld < 0 || (uint64_t)m2_ld < d) return fail(D3P_E_INVALID_ARG, "%s: m2_ld >= d is required", what);
    const uint32_t R = cm_segment_rows(n, d), nseg = cm_segments(n, R), nb = cm_blocks(d);
    const uint64_t pairs = cm_pairs(d), groups = pairs * nseg;
    if (groups > 0x7fffffffull)
        return fail(D3P_E_UNSUPPORTED, "%s: %llu block pairs x %u segments of rows = %llu workgroups, more than 2^31 - 1", what,
                    (unsigned long long)pairs, nseg, (unsigned long long)groups);
    const size_t need = cm_workspace(n, d);
    if (ws_bytes < need) return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_bytes, need);
    if (!is_device_ptr(x_dev) || !is_device_ptr(mean_dev) || !is_device_ptr(m2_dev) || !is_device_ptr(ws_dev))
        return fail(D3P_E_INVALID_ARG, "%s: the table, the outputs and the workspace must be device memory", what);
    const size_t dpad = (size_t)nb * D3P_CM_BLOCK;
    CmArgs a;
    a.x = static_cast<const uint32_t*>(x_dev); a.dtype = dtype; a.ld = ld; a.n = (uint32_t)n; a.d = d; a.nb = nb; a.nseg = nseg; a.R = R; a.sum_R = cm_sum_rows(n); a.sum_nseg = cm_segments(n, a.sum_R);
    a.npairs = pairs;
    a.shift = static_cast<float*>(ws_dev);
    a.flag = reinterpret_cast<uint32_t*>(a.shift + dpad);
    a.colsum = reinterpret_cast<double*>(a.flag + dpad);
    a.sums = a.colsum + (size_t)a.sum_nseg * dpad;
    a.parts = a.sums + pairs * 2u * D3P_CM_BLOCK;
    a.mean = mean_dev; a.m2 = m2_dev; a.m2_ld = m2_ld;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cm_colsum, dim3((unsigned)(dpad / D3P_CM_SUMCOLS), a.sum_nseg), dim3(256), 0, s, a);
    int rc = check_launch(what);
    if (rc != D3P_OK) return rc;
    hipLaunchKernelGGL(k_cm_shift, dim3((unsigned)(dpad / 32u)), dim3(256), 0, s, a);
    if ((rc = check_launch(what)) != D3P_OK) return rc;
    hipLaunchKernelGGL(k_cm_products, dim3((unsigned)pairs, nseg), dim3(64 * D3P_CM_WAVES), 0, s, a);
    if ((rc = check_launch(what)) != D3P_OK) return rc;
    hipLaunchKernelGGL(k_cm_sums, dim3((unsigned)pairs), dim3(2u * D3P_CM_BLOCK * D3P_CM_CHUNKS), 0, s, a);
    if ((rc = check_launch(what)) != D3P_OK) return rc;
    hipLaunchKernelGGL(k_cm_finish, dim3((unsigned)pairs, D3P_CM_G / 32u), dim3(256), 0, s, a);
    return check_launch(what);
}

}  // extern "C"
