// The two kernels of the sliced Wasserstein distance (d3p_amd/sliced.py, include/d3p_hip.h): the projection of a table's
// rows onto L directions on the matrix cores, written in the row-major layout d3p_sort_columns reads, and the squared 2-Wasserstein
// distance per column of two SORTED tables of unequal length.  The entries d3p_project_rows and d3p_column_w2_distance with their host
// checks, and the query functions of their geometry.  This file names no order key: it reads stored words only.
//
// ---- d3p_project_rows --------------------------------------------------------------------------------------------------------------------
// THE RULE.  x[i * ld + c] is row i < n in column c < d, float32 (dtype 0) or int32 (dtype 1: converted to float32 when loaded, exact for
// |v| <= 2^24, which is what the Python layer admits); theta[c * ld_t + l] is direction l < L; shift[c] a float32 per column, or no
// shift at all (a null pointer: t = x).
//     t_ic = fl32(x_ic - shift_c)                       (one float32 subtraction on the way into LDS)
//     p[i * ld_p + l] = sum_c t_ic theta_cl             (v_mfma_f32_32x32x2_f32, float32 accumulators: THE ORDER)
// THE ORDER, which is ONE order.  With K = 32 (d3p_project_rows_chunk_cols) the columns are cut into CHUNKS of K and a chunk into 16
// PAIRS (2 q, 2 q + 1).  p_il starts at +0 in an accumulator register of the matrix instruction; the chunks are taken in ascending
// order, within a chunk the pairs in ascending order, and pair q is ONE instruction acc <- acc + t_i,2q theta_2q,l + t_i,2q+1 theta_2q+1,l
// (how the instruction orders and rounds its two products and two additions is not documented; the bound below holds for any order
// with or without rounded products).  The last chunk is padded to K with t = 0 and theta = 0, so dp = K ceil(d / K) columns meet.
// p_il is a function of row i, column l of theta, shift, d and the dtype alone: not of n, ld, ld_p, ld_t, L, the other rows or
// directions, the tile of 32 rows or 32 directions it fell into, the slab of directions, or which of the two load forms ran.
// BOUND, against the float64 dot product of the same float32 t and theta, u = 2^-24, gamma_m = m u / (1 - m u):
//     |p^ - p| <= gamma_dp sum_c |t_ic| |theta_cl| + dp 2^-126
// The first term is Higham's bound for a dot product of dp terms with rounded products, summed in any order (a fused product only
// removes roundings); the second allows every product or partial sum that is subnormal to be flushed to zero (2^-126 each, dp of them
// at most lie on one result).  Overflow follows IEEE.
// NaN RULE.  A NaN in a row's d columns gives NaN in every projection of that row (NaN times any theta is NaN) and touches no other
// row; infinities follow IEEE (both signs, or an infinity against a theta of 0: NaN).
//
// THE KERNEL (k_project_rows).  The contraction runs over the COLUMNS, so the A operand of the matrix instruction -- lane l supplies row
// l % 32 at k = l / 32 -- wants 32 different rows at two columns: fed from global memory that is 8 bytes per row per instruction.  So
// both operands are staged in LDS.  A workgroup of four wavefronts owns a STRIP of R = 128 rows (d3p_project_rows_tile_rows), 32 per
// wavefront, and a SLAB of up to 128 directions (d3p_project_rows_max_launch_dirs); the grid is one-dimensional, strip-major, the slab
// fastest (a second grid dimension ends at 65535).  Per chunk:
//   * each wavefront loads ITS 32 rows x 32 columns: 16-byte loads along the row (8 lanes cover a row's 128 bytes, a wavefront 8 rows a
//     pass, 4 passes) when the table's address and ld allow them (16-byte aligned, ld a multiple of 4), else one word per lane (a
//     half-wave covers a row, 16 passes): 16 words per lane either way.  Shift subtracted, dead rows and columns zeroed by select AFTER
//     the subtraction, stored with a row pitch of 33 words, so that the operand read x_lds[l % 32][2 q + l / 32] of a half-wave hits
//     32 distinct banks.
//   * theta's chunk (32 x 128 words) is staged once per workgroup, one word per thread and pass (a row of 128 directions is 512
//     contiguous bytes), with a row pitch of 160 words: the read theta_lds[2 q + l / 32][32 j + l % 32] is contiguous over a half-wave
//     and the two halves are 32 banks apart.
//   * one A read feeds up to four matrix instructions (direction tiles j = 0 .. 3 of the slab: 64 accumulator registers).
//   * the NEXT chunk's global loads (16 + 16 words a lane) are issued before the current chunk's products and held in registers; LDS is
//     single-buffered, two barriers a chunk.
// LDS: 4 x 32 x 33 + 32 x 160 words = 37376 bytes, STATIC.  The choice: a chunk of 32 columns and no dynamic-LDS opt-in (a chunk of 64
// columns needs 65 KiB and with it the opt-in, which lives in the column reducers' header and its users are a fixed list); four
// workgroups fit a CU's 160 KiB.  A lane of a dead row reads the table's last row, of a dead column column 0, of a dead direction
// direction 0: every load is inside the table or theta and none sits behind a divergent branch.  Nothing outside p[i][0 .. L), i < n,
// is written.  No atomics, no scratch, no workspace, no host synchronisation, no allocation.
//
// ---- d3p_column_w2_distance --------------------------------------------------------------------------------------------------------------
// THE RULE.  a is d x ld_a with n_a sorted values per column, b is d x ld_b with n_b (d3p_sort_columns' output; float32 or int32, one
// dtype).  The quantile functions of a column are step functions on the integer grid of n_a n_b LEVELS: element i of a covers the levels
// [i n_b, (i + 1) n_b), element j of b covers [j n_a, (j + 1) n_a), and
//     w2sq[c] = (1 / (n_a n_b)) sum over the pairs (i, j) whose levels overlap of  overlap (a_(i) - b_(j))^2
// THE WALK has no search and no merge loop.  The entry names the LONGER column a (n_a >= n_b; with equal lengths nothing is swapped and
// the terms are symmetric), so element i meets j0 = floor(i n_b / n_a) and at most j1 = j0 + 1 = floor(((i + 1) n_b - 1) / n_a) <= n_b -
// 1.  With r = i n_b - j0 n_a the overlaps are the exact integers ov0 = min(n_a - r, n_b) and, when ov0 < n_b, ov1 = n_b - ov0.  A thread
// makes ONE 64-bit division (its first i) and steps r += n_b, with a carry into j0, from there.
// ORDER.  A term is three float64 roundings: delta = (double)a - (double)b, delta delta, times (double)overlap (exact: <= n_b < 2^31).  A
// block is D3P_CS_T = 4096 consecutive i of one column; thread t of 256 owns the D3P_CS_THREAD_KEYS = 16 consecutive i from block 4096 +
// 16 t and adds, in ascending i, the j0 term and then the j1 term onto +0; the threads merge in the tree red[t] += red[t + w], w = 128 ..
// 1; the blocks' partials go to the workspace and a second launch (one thread per column) adds them in ascending order onto +0 and
// divides ONCE by (double)n_a (double)n_b.  BOUND: |w2sq - exact| <= gamma_k sum |term| / (n_a n_b), k = 3 (a term) +
// d3p_column_w2_distance_roundings(n_a, n_b) = 32 (a thread's chain) + 8 (the tree) + the blocks of the longer column (the merge) + 2 (the
// denominator and the division), gamma_k = k u / (1 - k u), u = 2^-53.  Equal tables give exactly 0.
// NON-FINITE RULE, one test at the ends: by the sort's order a float32 column holds a NaN or an infinity exactly when its first or its
// last stored word is not finite; such a column, in either table, gives w2sq = NaN and touches no other column.  int32 is always finite.
// Workspace: 8 bytes per (column, block of the longer column); every word read is written before in the same call.  No atomics, no
// scratch, static LDS (2 KiB), plain float64 loads and stores in the tree.
#include "d3p_device.h"
#include "d3p_host.h"
#include "d3p_sort_columns.h"

#define D3P_PR_WAVES 4u
#define D3P_PR_TILE 32u                                   // rows of a wavefront, directions of a tile
#define D3P_PR_STRIP (D3P_PR_WAVES * D3P_PR_TILE)         // R: rows of a workgroup (d3p_project_rows_tile_rows)
#define D3P_PR_CHUNK 32u                                  // K: columns staged at a time (d3p_project_rows_chunk_cols)
#define D3P_PR_JT 4u                                      // direction tiles of a wavefront
#define D3P_PR_DIRS (D3P_PR_JT * D3P_PR_TILE)             // directions of a slab (d3p_project_rows_max_launch_dirs)
#define D3P_PR_XPITCH (D3P_PR_CHUNK + 1u)
#define D3P_PR_TPITCH (D3P_PR_DIRS + 32u)
#define D3P_PR_WORDS 16u                                  // words of the table, and of theta, a lane holds for the next chunk

namespace d3p {

typedef float pr_f16v __attribute__((ext_vector_type(16)));

struct PrArgs {
    const uint32_t* x; int32_t dtype; int64_t ld; uint32_t n, d;
    const float* theta; int64_t ld_t; uint32_t L;
    const float* shift;      // or null
    float* p; int64_t ld_p;
    uint32_t nslab;          // ceil(L / D3P_PR_DIRS)
};

__device__ __forceinline__ float pr_value(int32_t dtype, uint32_t w) { return dtype ? (float)(int32_t)w : __uint_as_float(w); }

// VEC: the table is read with 16-byte loads (its address is 16-byte aligned and ld is a multiple of 4, so a group of four columns that
// starts below d ends below ld); else one word a lane.  The arithmetic, and so every bit of p, is the same.
template <bool VEC>
__global__ __launch_bounds__(64 * D3P_PR_WAVES) void k_project_rows(PrArgs a)
{
    __shared__ float xs[D3P_PR_WAVES][D3P_PR_TILE * D3P_PR_XPITCH];
    __shared__ float ts[D3P_PR_CHUNK * D3P_PR_TPITCH];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, half = lane >> 5, sub = lane & 31u;
    const uint32_t strip = blockIdx.x / a.nslab, slab = blockIdx.x % a.nslab;
    const uint32_t r0 = strip * D3P_PR_STRIP + wave * D3P_PR_TILE;    // the wavefront's first row (n < 2^31: no wrap)
    const uint32_t l0 = slab * D3P_PR_DIRS;
    const uint32_t ndir = a.L - l0 < D3P_PR_DIRS ? a.L - l0 : D3P_PR_DIRS, ntile = (ndir + D3P_PR_TILE - 1u) / D3P_PR_TILE;
    const uint32_t nchunk = (a.d + D3P_PR_CHUNK - 1u) / D3P_PR_CHUNK;
    // the lane's place in its wavefront's tile of the table: (row of pass p, first column) = VEC: (8 p + lane / 8, 4 (lane % 8)), else
    // (2 p + half, sub); in theta's chunk: (row 2 p + t / 128, direction t % 128)
    const uint32_t xrow = VEC ? lane >> 3 : half, xcol = VEC ? 4u * (lane & 7u) : sub, xstep = VEC ? 8u : 2u;
    const uint32_t trow = t >> 7, tcol = t & 127u;
    const bool dir_live = l0 + tcol < a.L;
    const float* tbase = a.theta + (dir_live ? l0 + tcol : 0u);
    uint32_t xw[D3P_PR_WORDS];
    float tw[D3P_PR_WORDS], sh[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float* mine = xs[wave];

    auto load = [&](uint32_t c0) {
        const uint32_t cb = c0 + xcol;
        if (VEC) {
            const uint32_t cr = cb < a.d ? cb : 0u;
#pragma unroll
            for (uint32_t p = 0; p < 4u; ++p) {
                const uint32_t row = r0 + xstep * p + xrow;
                const uint4 v = *reinterpret_cast<const uint4*>(a.x + (int64_t)(row < a.n ? row : a.n - 1u) * a.ld + cr);
                xw[4u * p] = v.x; xw[4u * p + 1u] = v.y; xw[4u * p + 2u] = v.z; xw[4u * p + 3u] = v.w;
            }
        } else {
            const uint32_t cr = cb < a.d ? cb : 0u;
#pragma unroll
            for (uint32_t p = 0; p < D3P_PR_WORDS; ++p) {
                const uint32_t row = r0 + xstep * p + xrow;
                xw[p] = a.x[(int64_t)(row < a.n ? row : a.n - 1u) * a.ld + cr];
            }
        }
        if (a.shift) {    // (uniform)
#pragma unroll
            for (uint32_t e = 0; e < (VEC ? 4u : 1u); ++e) sh[e] = a.shift[cb + e < a.d ? cb + e : 0u];
        }
#pragma unroll
        for (uint32_t p = 0; p < D3P_PR_WORDS; ++p) {
            const uint32_t k = c0 + 2u * p + trow;
            tw[p] = tbase[(int64_t)(k < a.d ? k : 0u) * a.ld_t];
        }
    };
    auto store = [&](uint32_t c0) {
        const uint32_t cb = c0 + xcol;
        if (VEC) {
#pragma unroll
            for (uint32_t p = 0; p < 4u; ++p) {
                const uint32_t lr = xstep * p + xrow;
                const bool row_live = r0 + lr < a.n;
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e) {
                    const float v = pr_value(a.dtype, xw[4u * p + e]) - sh[e];
                    mine[lr * D3P_PR_XPITCH + xcol + e] = (row_live && cb + e < a.d) ? v : 0.0f;
                }
            }
        } else {
#pragma unroll
            for (uint32_t p = 0; p < D3P_PR_WORDS; ++p) {
                const uint32_t lr = xstep * p + xrow;
                const float v = pr_value(a.dtype, xw[p]) - sh[0];
                mine[lr * D3P_PR_XPITCH + xcol] = (r0 + lr < a.n && cb < a.d) ? v : 0.0f;
            }
        }
#pragma unroll
        for (uint32_t p = 0; p < D3P_PR_WORDS; ++p) {
            const uint32_t kr = 2u * p + trow;
            ts[kr * D3P_PR_TPITCH + tcol] = (dir_live && c0 + kr < a.d) ? tw[p] : 0.0f;
        }
    };

    pr_f16v acc[D3P_PR_JT];
#pragma unroll
    for (uint32_t j = 0; j < D3P_PR_JT; ++j)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[j][v] = 0.0f;
    load(0u);
    for (uint32_t c = 0; c < nchunk; ++c) {
        if (c) __syncthreads();          // the products of the chunk before have read LDS
        store(c * D3P_PR_CHUNK);
        __syncthreads();
        if (c + 1u < nchunk) load((c + 1u) * D3P_PR_CHUNK);
#pragma unroll
        for (uint32_t q = 0; q < D3P_PR_CHUNK / 2u; ++q) {
            const float av = mine[sub * D3P_PR_XPITCH + 2u * q + half];
            const float* brow = ts + (2u * q + half) * D3P_PR_TPITCH + sub;
#pragma unroll
            for (uint32_t j = 0; j < D3P_PR_JT; ++j)
                if (j < ntile) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, brow[D3P_PR_TILE * j], acc[j], 0, 0, 0);   // (uniform)
        }
    }
    // register v of lane (half, sub) is D[8 (v / 4) + 4 half + v % 4][sub]: a half-wave writes 32 consecutive directions of one row
#pragma unroll
    for (uint32_t j = 0; j < D3P_PR_JT; ++j) {
        const uint32_t l = l0 + D3P_PR_TILE * j + sub;
        if (j < ntile && l < a.L) {
#pragma unroll
            for (uint32_t v = 0; v < 16u; ++v) {
                const uint32_t row = r0 + 8u * (v >> 2) + 4u * half + (v & 3u);
                if (row < a.n) a.p[(int64_t)row * a.ld_p + l] = acc[j][v];
            }
        }
    }
}

struct W2Args {
    const uint32_t* a; const uint32_t* b;   // a: the longer column (n_a >= n_b)
    int64_t ld_a, ld_b; uint32_t n_a, n_b, d; int32_t dtype; uint32_t nblk;   // nblk: the blocks of a
    double* part;    // d x nblk
    double* out;     // d
};

__device__ __forceinline__ double w2_value(int32_t dtype, uint32_t w) { return dtype ? (double)(int32_t)w : (double)__uint_as_float(w); }

__global__ __launch_bounds__(256) void k_w2_part(W2Args g)
{
#pragma clang fp contract(off)
    __shared__ double red[256];
    const uint32_t c = blockIdx.x / g.nblk, blk = blockIdx.x % g.nblk, t = threadIdx.x;
    const uint32_t* ca = g.a + (size_t)c * (size_t)g.ld_a;
    const uint32_t* cb = g.b + (size_t)c * (size_t)g.ld_b;
    const uint64_t na = g.n_a, nb = g.n_b;
    uint64_t i = (uint64_t)blk * D3P_CS_T + (uint64_t)t * D3P_CS_THREAD_KEYS;
    double acc = 0.0;
    if (i < na) {
        const uint64_t hi = i + D3P_CS_THREAD_KEYS < na ? i + D3P_CS_THREAD_KEYS : na;
        uint64_t j = i * nb / na, r = i * nb - j * na;     // element i starts r levels into element j of b (i n_b < 2^62)
        for (; i < hi; ++i) {
            const double av = w2_value(g.dtype, ca[i]);
            const uint64_t room = na - r, ov0 = room < nb ? room : nb;
            const double d0 = av - w2_value(g.dtype, cb[j]);
            const double s0 = d0 * d0;
            acc = acc + s0 * (double)ov0;
            if (ov0 < nb) {                                  // (then j + 1 <= n_b - 1: the header)
                const double d1 = av - w2_value(g.dtype, cb[j + 1u]);
                const double s1 = d1 * d1;
                acc = acc + s1 * (double)(nb - ov0);
            }
            r += nb;
            if (r >= na) { r -= na; ++j; }
        }
    }
    red[t] = acc;
    __syncthreads();
    for (uint32_t w = 128u; w > 0u; w >>= 1) {
        if (t < w) red[t] = red[t] + red[t + w];
        __syncthreads();
    }
    if (t == 0u) g.part[(size_t)c * g.nblk + blk] = red[0];
}

__device__ __forceinline__ bool w2_finite(uint32_t w) { return (w & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(64) void k_w2_merge(W2Args g)
{
#pragma clang fp contract(off)
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= g.d) return;
    const uint32_t* ca = g.a + (size_t)c * (size_t)g.ld_a;
    const uint32_t* cb = g.b + (size_t)c * (size_t)g.ld_b;
    const bool bad = !g.dtype && !(w2_finite(ca[0]) && w2_finite(ca[g.n_a - 1u]) && w2_finite(cb[0]) && w2_finite(cb[g.n_b - 1u]));
    double s = 0.0;
    for (uint32_t b = 0; b < g.nblk; ++b) s = s + g.part[(size_t)c * g.nblk + b];
    const double denom = (double)g.n_a * (double)g.n_b;
    g.out[c] = bad ? (double)NAN : s / denom;
}

static const uint64_t SL_MAX_N = 0x7fffffffull;        // 2^31 - 1
static const uint64_t SL_MAX_GROUPS = 0x7fffffffull;

static bool sl_mul_fits(uint64_t a, uint64_t b) { return b == 0 || a <= (uint64_t)INT64_MAX / b; }

static size_t w2_workspace(uint64_t n_a, uint64_t n_b, uint32_t d)
{
    if (n_a < 1 || n_a > SL_MAX_N || n_b < 1 || n_b > SL_MAX_N || d < 1) return 0;
    const uint64_t parts = (uint64_t)d * cs_blocks(n_a > n_b ? n_a : n_b);
    if (parts > SL_MAX_GROUPS) return 0;
    return (size_t)(parts * 8u);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_project_rows_tile_rows(void) { return D3P_PR_STRIP; }

uint32_t d3p_project_rows_chunk_cols(void) { return D3P_PR_CHUNK; }

uint32_t d3p_project_rows_max_launch_dirs(void) { return D3P_PR_DIRS; }

int d3p_project_rows(void* stream, const void* x_dev, int32_t dtype, int64_t ld, uint64_t n, uint32_t d, const float* theta_dev, int64_t ld_t,
                     uint32_t L, const float* shift_dev, float* p_dev, int64_t ld_p)
{
    const char* what = "d3p_project_rows";
    if (!x_dev || !theta_dev || !p_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)x_dev | (uintptr_t)theta_dev | (uintptr_t)shift_dev | (uintptr_t)p_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (d < 1) return fail(D3P_E_INVALID_ARG, "%s: d >= 1 is required", what);
    if (ld < 0 || (uint64_t)ld < d) return fail(D3P_E_INVALID_ARG, "%s: ld >= d is required", what);
    if (ld_p < 0 || (uint64_t)ld_p < L) return fail(D3P_E_INVALID_ARG, "%s: ld_p >= L is required", what);
    if (ld_t < 0 || (uint64_t)ld_t < L) return fail(D3P_E_INVALID_ARG, "%s: ld_t >= L is required", what);
    if (!sl_mul_fits(n, (uint64_t)ld) || !sl_mul_fits(n, (uint64_t)ld_p) || !sl_mul_fits(d, (uint64_t)ld_t))
        return fail(D3P_E_INVALID_ARG, "%s: n * ld, n * ld_p or d * ld_t does not fit 63 bits", what);
    if (n > SL_MAX_N) return fail(D3P_E_UNSUPPORTED, "%s: %llu rows; at most 2^31 - 1", what, (unsigned long long)n);
    const uint64_t strips = (n + D3P_PR_STRIP - 1u) / D3P_PR_STRIP, nslab = ((uint64_t)L + D3P_PR_DIRS - 1u) / D3P_PR_DIRS, groups = strips * nslab;
    if (groups > SL_MAX_GROUPS)
        return fail(D3P_E_UNSUPPORTED, "%s: %llu strips of rows x %llu slabs of directions = %llu workgroups, more than 2^31 - 1", what,
                    (unsigned long long)strips, (unsigned long long)nslab, (unsigned long long)groups);
    if (n == 0 || L == 0) return D3P_OK;
    if (!is_device_ptr(x_dev) || !is_device_ptr(theta_dev) || !is_device_ptr(p_dev) || (shift_dev && !is_device_ptr(shift_dev)))
        return fail(D3P_E_INVALID_ARG, "%s: the table, the directions, the shift and the output must be device memory", what);
    PrArgs a;
    a.x = static_cast<const uint32_t*>(x_dev); a.dtype = dtype; a.ld = ld; a.n = (uint32_t)n; a.d = d;
    a.theta = theta_dev; a.ld_t = ld_t; a.L = L; a.shift = shift_dev; a.p = p_dev; a.ld_p = ld_p; a.nslab = (uint32_t)nslab;
    const bool vec = ((uintptr_t)x_dev & 15u) == 0 && (ld & 3) == 0;
    if (vec)
        hipLaunchKernelGGL(k_project_rows<true>, dim3((unsigned)groups), dim3(64 * D3P_PR_WAVES), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_project_rows<false>, dim3((unsigned)groups), dim3(64 * D3P_PR_WAVES), 0, (hipStream_t)stream, a);
    return check_launch(what);
}

size_t d3p_column_w2_distance_workspace(uint64_t n_a, uint64_t n_b, uint32_t d) { return w2_workspace(n_a, n_b, d); }

uint32_t d3p_column_w2_distance_roundings(uint64_t n_a, uint64_t n_b)
{
    if (n_a < 1 || n_a > SL_MAX_N || n_b < 1 || n_b > SL_MAX_N) return 0u;
    return 2u * D3P_CS_THREAD_KEYS + 8u + cs_blocks(n_a > n_b ? n_a : n_b) + 2u;   // a thread's chain; the tree of 256; the merge; the denominator, the division
}

int d3p_column_w2_distance(void* stream, const void* a_dev, int64_t ld_a, uint64_t n_a, const void* b_dev, int64_t ld_b, uint64_t n_b,
                           int32_t dtype, uint32_t d, double* w2sq_dev, void* ws_dev, size_t ws_bytes)
{
    const char* what = "d3p_column_w2_distance";
    if (!a_dev || !b_dev || !w2sq_dev || !ws_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)a_dev | (uintptr_t)b_dev) & 3u) != 0) return fail(D3P_E_INVALID_ARG, "%s: a_dev or b_dev is not aligned to 4 bytes", what);
    if ((((uintptr_t)w2sq_dev | (uintptr_t)ws_dev) & 7u) != 0) return fail(D3P_E_INVALID_ARG, "%s: w2sq_dev or ws_dev is not aligned to 8 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (n_a < 1 || n_a > SL_MAX_N || n_b < 1 || n_b > SL_MAX_N)
        return fail(D3P_E_INVALID_ARG, "%s: 1 <= n_a, n_b <= 2^31 - 1 are required (n_a n_b < 2^63)", what);
    if (d < 1) return fail(D3P_E_INVALID_ARG, "%s: d >= 1 is required", what);
    if (ld_a < 0 || (uint64_t)ld_a < n_a || ld_b < 0 || (uint64_t)ld_b < n_b)
        return fail(D3P_E_INVALID_ARG, "%s: ld_a >= n_a and ld_b >= n_b are required", what);
    if (!sl_mul_fits(d, (uint64_t)ld_a) || !sl_mul_fits(d, (uint64_t)ld_b))
        return fail(D3P_E_INVALID_ARG, "%s: d * ld_a or d * ld_b does not fit 63 bits", what);
    const bool swap = n_b > n_a;
    const uint32_t nblk = cs_blocks(swap ? n_b : n_a);
    const uint64_t parts = (uint64_t)d * nblk;
    if (parts > SL_MAX_GROUPS)
        return fail(D3P_E_UNSUPPORTED, "%s: %u columns x %u blocks of positions = %llu workgroups, more than 2^31 - 1", what, d, nblk,
                    (unsigned long long)parts);
    const size_t need = w2_workspace(n_a, n_b, d);
    if (ws_bytes < need) return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_bytes, need);
    if (!is_device_ptr(a_dev) || !is_device_ptr(b_dev) || !is_device_ptr(w2sq_dev) || !is_device_ptr(ws_dev))
        return fail(D3P_E_INVALID_ARG, "%s: the tables, the output and the workspace must be device memory", what);
    W2Args g;
    g.a = static_cast<const uint32_t*>(swap ? b_dev : a_dev); g.b = static_cast<const uint32_t*>(swap ? a_dev : b_dev);
    g.ld_a = swap ? ld_b : ld_a; g.ld_b = swap ? ld_a : ld_b;
    g.n_a = (uint32_t)(swap ? n_b : n_a); g.n_b = (uint32_t)(swap ? n_a : n_b); g.d = d; g.dtype = dtype; g.nblk = nblk;
    g.part = static_cast<double*>(ws_dev); g.out = w2sq_dev;
    hipLaunchKernelGGL(k_w2_part, dim3((unsigned)parts), dim3(256), 0, (hipStream_t)stream, g);
    const int rc = check_launch(what);
    if (rc != D3P_OK) return rc;
    hipLaunchKernelGGL(k_w2_merge, dim3((d + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, g);
    return check_launch(what);
}

}  // extern "C"
