// Binned one- and two-way marginal counts of a table (d3p_amd/marginals.py, include/d3p_hip.h): per column the histogram of
// its discretised values and per pair of columns i < j their contingency table -- what the total variation distance of the 1- and 2-way
// marginals and the pairwise association (Cramer's V) of a synthetic table against the real one reduce.  The entry d3p_marginals with its
// host checks, its two kernels and the query functions of their constants and workspace.
//
// THE RULE.  x[r * ld + c] is row r < n of the table in column c < d, float32 (dtype 0) or int32 (dtype 1: converted to float32 when
// staged, exact for |v| <= 2^24, which is what the Python layer admits).  Column c has nb_c = nbins[c] bins, 1 <= nb_c <= B, cut by
// m = nb_c - 1 finite, non-decreasing float32 edges e_0 <= .. <= e_{m-1} = edges[c * (B - 1) + k]; B <= d3p_marginals_max_bins() = 32.
// The CODE of a value v in column c:
//     v is NaN                  -> B, the MISSING cell
//     otherwise                 -> #{k < m : e_k < v}            (numpy's searchsorted(e, v, side="left"))
// so the bins are right-closed: bin 0 holds everything <= e_0, -inf included, the last bin everything above e_{m-1}, +inf included, and
// -0.0 and 0.0 are equal.  The CELL STRIDE is K = B + 1.  Both outputs are uint32 (n <= 2^32 - 1 fits):
//     one_way[c * K + u]           = #{r : code(r, c) == u}
//     two_way[(p * K + u) * K + v] = #{r : code(r, i) == u and code(r, j) == v}     for the pair i < j with the lexicographic index
//                                    p = i (2 d - i - 1) / 2 + (j - i - 1)
// The entry zeroes both outputs itself; d = 1 has no pairs (two_way may then be null).  The outputs are integers: a function of the
// arguments alone, whatever the grid, the replica a lane adds to or the order of the atomic adds.
//
// SAFETY.  nbins and edges are device memory the host entry cannot read.  The kernel clamps nb_c into [1, B] and its search visits at
// most B - 1 entries of column c's own B - 1 edge slots, so every code lies in [0, B] BY CONSTRUCTION, whatever those arrays hold;
// unsorted edges give an unspecified but in-range code.  The Python layer checks finiteness and order on the host before any launch.
//
// HOW.  Two launches, one form.
//   1. k_marginal_codes writes the uint8 code of every element to the workspace, COLUMN-major (codes[c * n + r]: the pair walk reads one
//      column's codes of consecutive rows), through a transposing LDS tile of 4096 elements (2^w columns x 4096 / 2^w rows, 2^w the
//      power of two >= min(d, 64)), so the table is read along its rows and the codes are written along theirs.  A workgroup owns
//      d3p_marginals_code_rows() = 4096 rows of up to 64 columns, keeps those columns' one-way histograms in LDS and flushes the non-zero
//      cells with integer atomicAdd.  The workspace is exactly n * d bytes (d3p_marginals_workspace) and every byte of it is written
//      here before the second launch reads it: its contents on entry change nothing.
//   2. k_marginal_pairs gives a workgroup d3p_marginals_pair_tile() = 4 consecutive pairs and a strip of d3p_marginals_strip_rows() =
//      32768 rows.  Its LDS holds R replicas of the tile's 4 K^2 uint32 cells, R = min(16, 15360 / (4 K^2)) (3 at B = 32, 13 at B = 16);
//      lane l adds to replica l mod R, so the lanes of a wavefront that meet on ONE cell -- a categorical column with a dominant value
//      -- serialise over 64 / R lanes and not 64.  After the strip the replicas are summed and the non-zero cells go to two_way by integer
//      atomicAdd (the precedent: d3p_classify.hip).  The flush reads 4 R K^2 <= 15360 LDS words per strip beside 4 x 32768 increments.
//      A 32-bit LDS counter sees at most 32768 increments: none can overflow.
// Static LDS: 61440 bytes (pairs), 20800 bytes (codes).  No scratch, no floating-point atomics, no dynamic LDS, no host synchronisation.
#include "d3p_device.h"
#include "d3p_host.h"

#define D3P_MG_MAX_BINS 32
#define D3P_MG_STRIP 32768u       // rows of a strip of the pair walk
#define D3P_MG_PT 4u              // pairs a workgroup of the pair walk holds at once
#define D3P_MG_HIST_WORDS 15360u  // LDS words of the replicated pair histograms
#define D3P_MG_MAX_REP 16u
#define D3P_MG_CODE_ROWS 4096u    // rows a workgroup of the code kernel owns
#define D3P_MG_TILE 4096u         // elements of its transposing tile
#define D3P_MG_TC 64u             // columns of a column block

namespace d3p {

struct MgArgs {
    const uint32_t* x; int32_t dtype; int64_t ld; uint32_t n, d, B;
    const uint32_t* nbins; const float* edges;
    uint32_t* one_way; uint32_t* two_way; uint8_t* codes;
    uint64_t pairs; uint32_t strips, rep;
};

// launch 1: codes and one-way counts.  blockIdx.x = row block + row blocks x column block.
__global__ __launch_bounds__(256) void k_marginal_codes(MgArgs a)
{
    __shared__ float s_edge[D3P_MG_TC * (D3P_MG_MAX_BINS - 1)];
    __shared__ uint32_t s_m[D3P_MG_TC];                               // edges searched per column: clamp(nbins, 1, B) - 1
    __shared__ uint32_t s_hist[D3P_MG_TC * (D3P_MG_MAX_BINS + 1)];
    __shared__ uint8_t s_tile[D3P_MG_TILE + D3P_MG_TC];               // [column][rows of the tile + 1]
    const uint32_t tid = threadIdx.x, K = a.B + 1u, E = a.B - 1u;
    const uint32_t row_blocks = (uint32_t)(((uint64_t)a.n + D3P_MG_CODE_ROWS - 1u) / D3P_MG_CODE_ROWS);
    const uint32_t col0 = (blockIdx.x / row_blocks) * D3P_MG_TC;
    const uint64_t row0 = (uint64_t)(blockIdx.x % row_blocks) * D3P_MG_CODE_ROWS;
    const uint32_t cw = a.d - col0 < D3P_MG_TC ? a.d - col0 : D3P_MG_TC;                     // columns of this block
    const uint32_t lw = cw > 32 ? 6 : cw > 16 ? 5 : cw > 8 ? 4 : cw > 4 ? 3 : cw > 2 ? 2 : cw > 1 ? 1 : 0;
    const uint32_t tr = D3P_MG_TILE >> lw, ts = tr + 1u;                                     // rows of a tile, its LDS stride
    if (tid < D3P_MG_TC) {
        uint32_t nb = tid < cw ? a.nbins[col0 + tid] : 1u;
        nb = nb < 1u ? 1u : nb > a.B ? a.B : nb;
        s_m[tid] = nb - 1u;
    }
    for (uint32_t e = tid; e < cw * E; e += 256u) s_edge[e] = a.edges[(size_t)col0 * E + e];  // column col0 + e / E, edge e % E
    for (uint32_t e = tid; e < D3P_MG_TC * K; e += 256u) s_hist[e] = 0u;
    __syncthreads();
    const uint64_t row_end = row0 + D3P_MG_CODE_ROWS < a.n ? row0 + D3P_MG_CODE_ROWS : a.n;
    for (uint64_t t0 = row0; t0 < row_end; t0 += tr) {
#pragma unroll 4
        for (uint32_t k = 0; k < D3P_MG_TILE / 256u; ++k) {          // along the rows of the table
            const uint32_t e = k * 256u + tid, c = e & ((1u << lw) - 1u), r = e >> lw;
            const uint64_t row = t0 + r;
            if (c < cw && row < row_end) {
                const uint32_t w = a.x[(int64_t)row * a.ld + col0 + c];
                const float v = a.dtype ? (float)(int32_t)w : __uint_as_float(w);
                const float* ed = s_edge + c * E;
                uint32_t lo = 0u, hi = s_m[c];                        // hi <= B - 1 <= 31: five halvings end the search
#pragma unroll
                for (int it = 0; it < 5; ++it) {
                    const uint32_t mid = (lo + hi) >> 1;              // < hi <= E while lo < hi: inside the column's own slots
                    const bool open = lo < hi;
                    const bool less = open && ed[open ? mid : 0u] < v;
                    lo = less ? mid + 1u : lo;
                    hi = open && !less ? mid : hi;
                }
                s_tile[c * ts + r] = (uint8_t)(v != v ? a.B : lo);
            }
        }
        __syncthreads();
#pragma unroll 4
        for (uint32_t k = 0; k < D3P_MG_TILE / 256u; ++k) {          // along the rows of the codes
            const uint32_t e = k * 256u + tid, r = e & (tr - 1u), c = e >> (12u - lw);
            const uint64_t row = t0 + r;
            if (c < cw && row < row_end) {
                const uint32_t code = s_tile[c * ts + r];
                a.codes[(size_t)(col0 + c) * a.n + row] = (uint8_t)code;
                atomicAdd(&s_hist[c * K + code], 1u);
            }
        }
        __syncthreads();
    }
    for (uint32_t e = tid; e < cw * K; e += 256u) {
        const uint32_t v = s_hist[e];
        if (v) atomicAdd(a.one_way + (size_t)col0 * K + e, v);
    }
}

__device__ __forceinline__ uint64_t mg_pair_start(uint64_t i, uint64_t d) { return i * (2u * d - i - 1u) / 2u; }

// launch 2: the pair walk.  blockIdx.x = strip + strips x pair tile.
__global__ __launch_bounds__(256) void k_marginal_pairs(MgArgs a)
{
    __shared__ uint32_t s_hist[D3P_MG_HIST_WORDS];
    const uint32_t tid = threadIdx.x, K = a.B + 1u, KK = K * K, cells = D3P_MG_PT * KK;
    const uint64_t p0 = (uint64_t)(blockIdx.x / a.strips) * D3P_MG_PT;
    const uint64_t row0 = (uint64_t)(blockIdx.x % a.strips) * D3P_MG_STRIP;
    const uint64_t row_end = row0 + D3P_MG_STRIP < a.n ? row0 + D3P_MG_STRIP : a.n;
    const uint32_t np = a.pairs - p0 < D3P_MG_PT ? (uint32_t)(a.pairs - p0) : D3P_MG_PT;
    // pair p0 = (i, j): the closed form of the lexicographic index, then set right by whole steps (d < 2^32: every term exact in float64)
    const uint64_t d = a.d;
    const double two_d1 = (double)(2u * d - 1u), disc = two_d1 * two_d1 - 8.0 * (double)p0;
    uint64_t i0 = (uint64_t)((two_d1 - sqrt(disc > 0.0 ? disc : 0.0)) * 0.5);
    i0 = i0 > d - 2u ? d - 2u : i0;
    while (i0 > 0u && mg_pair_start(i0, d) > p0) --i0;
    while (i0 + 2u < d && mg_pair_start(i0 + 1u, d) <= p0) ++i0;
    uint32_t pi[D3P_MG_PT], pj[D3P_MG_PT];
    {
        uint32_t i = (uint32_t)i0, j = (uint32_t)(i0 + 1u + (p0 - mg_pair_start(i0, d)));
#pragma unroll
        for (uint32_t q = 0; q < D3P_MG_PT; ++q) {
            pi[q] = q < np ? i : 0u;                                  // (a pair past the last one reads column 0 and adds nothing)
            pj[q] = q < np ? j : 0u;
            if (++j >= a.d) { ++i; j = i + 1u; }
        }
    }
    const uint32_t used = a.rep * cells;                              // <= D3P_MG_HIST_WORDS by the host's choice of rep
    for (uint32_t e = tid; e < used; e += 256u) s_hist[e] = 0u;
    __syncthreads();
    uint32_t* mine = s_hist + ((tid & 63u) % a.rep) * cells;
    for (uint64_t row = row0 + tid; row < row_end; row += 256u) {
        uint32_t ci[D3P_MG_PT], cj[D3P_MG_PT];
#pragma unroll
        for (uint32_t q = 0; q < D3P_MG_PT; ++q) {
            if (q > 0 && pi[q] == pi[q - 1]) ci[q] = ci[q - 1];
            else ci[q] = a.codes[(size_t)pi[q] * a.n + row];
            cj[q] = a.codes[(size_t)pj[q] * a.n + row];
        }
#pragma unroll
        for (uint32_t q = 0; q < D3P_MG_PT; ++q) {
            const uint32_t u = ci[q] > a.B ? a.B : ci[q], v = cj[q] > a.B ? a.B : cj[q];   // (the codes of launch 1 are <= B already)
            if (q < np) atomicAdd(mine + q * KK + u * K + v, 1u);
        }
    }
    __syncthreads();
    for (uint32_t e = tid; e < np * KK; e += 256u) {
        uint32_t s = 0u;
        for (uint32_t r = 0; r < a.rep; ++r) s += s_hist[r * cells + e];
        if (s) atomicAdd(a.two_way + (size_t)p0 * KK + e, s);
    }
}

static uint32_t mg_replicas(uint32_t B)
{
    const uint32_t K = B + 1u, r = D3P_MG_HIST_WORDS / (D3P_MG_PT * K * K);   // >= 3 for B <= 32
    return r > D3P_MG_MAX_REP ? D3P_MG_MAX_REP : r;
}

}  // namespace d3p

using namespace d3p;

static_assert(D3P_MG_PT * (D3P_MG_MAX_BINS + 1) * (D3P_MG_MAX_BINS + 1) <= D3P_MG_HIST_WORDS, "one replica of the widest tile fits");
static_assert(D3P_MG_TILE == 4096 && D3P_MG_CODE_ROWS % D3P_MG_TILE == 0 && D3P_MG_TC == 64, "k_marginal_codes' lane maps");

extern "C" {

uint32_t d3p_marginals_max_bins(void) { return D3P_MG_MAX_BINS; }

uint32_t d3p_marginals_strip_rows(void) { return D3P_MG_STRIP; }

uint32_t d3p_marginals_pair_tile(void) { return D3P_MG_PT; }

uint32_t d3p_marginals_code_rows(void) { return D3P_MG_CODE_ROWS; }

size_t d3p_marginals_workspace(uint32_t n, uint32_t d, uint32_t B)
{
    if (n < 1 || d < 1 || B < 1 || B > D3P_MG_MAX_BINS) return 0;
    return (size_t)n * (size_t)d;   // < 2^64: no wrap
}

int d3p_marginals(void* stream, const void* x_dev, int32_t dtype, int64_t ld, uint32_t n, uint32_t d, uint32_t B, const uint32_t* nbins_dev,
                  const float* edges_dev, uint32_t* one_way_dev, uint32_t* two_way_dev, void* ws_dev, size_t ws_bytes)
{
    const char* what = "d3p_marginals";
    if (!x_dev || !nbins_dev || !edges_dev || !one_way_dev || (d > 1 && !two_way_dev)) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)x_dev | (uintptr_t)nbins_dev | (uintptr_t)edges_dev | (uintptr_t)one_way_dev | (uintptr_t)two_way_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n >= 1 is required", what);
    if (d < 1) return fail(D3P_E_INVALID_ARG, "%s: d >= 1 is required", what);
    if (ld < 0 || (uint64_t)ld < d) return fail(D3P_E_INVALID_ARG, "%s: ld >= d is required", what);
    if ((uint64_t)n > (uint64_t)INT64_MAX / (uint64_t)ld) return fail(D3P_E_INVALID_ARG, "%s: n * ld does not fit 63 bits", what);
    if (B < 1 || B > D3P_MG_MAX_BINS)
        return fail(D3P_E_INVALID_ARG, "%s: 1 <= B <= %d bins are required, got %u", what, D3P_MG_MAX_BINS, B);
    const size_t need = (size_t)n * (size_t)d;
    if (ws_bytes < need || !ws_dev)
        return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_dev ? ws_bytes : (size_t)0, need);
    const uint64_t K = B + 1u, pairs = (uint64_t)d * (d - 1u) / 2u;
    const uint64_t strips = ((uint64_t)n + D3P_MG_STRIP - 1u) / D3P_MG_STRIP, tiles = (pairs + D3P_MG_PT - 1u) / D3P_MG_PT;
    const uint64_t row_blocks = ((uint64_t)n + D3P_MG_CODE_ROWS - 1u) / D3P_MG_CODE_ROWS, col_blocks = ((uint64_t)d + D3P_MG_TC - 1u) / D3P_MG_TC;
    if (tiles > 0x7fffffffull / strips || row_blocks * col_blocks > 0x7fffffffull)
        return fail(D3P_E_UNSUPPORTED, "%s: d = %u at n = %u needs more than 2^31 - 1 workgroups (one per %u pairs and %u rows)", what, d, n,
                    D3P_MG_PT, D3P_MG_STRIP);
    // (at most 2^33 pairs pass: their tables, below 2^46 bytes, fit size_t)
    if (!is_device_ptr(x_dev) || !is_device_ptr(nbins_dev) || !is_device_ptr(edges_dev) || !is_device_ptr(one_way_dev) ||
        (d > 1 && !is_device_ptr(two_way_dev)) || !is_device_ptr(ws_dev))
        return fail(D3P_E_INVALID_ARG, "%s: the table, nbins, edges, the outputs and the workspace must be device memory", what);
    hipStream_t s = (hipStream_t)stream;
    D3P_HIP_TRY(hipMemsetAsync(one_way_dev, 0, (size_t)d * K * sizeof(uint32_t), s));
    if (pairs) D3P_HIP_TRY(hipMemsetAsync(two_way_dev, 0, (size_t)pairs * K * K * sizeof(uint32_t), s));
    MgArgs a;
    a.x = static_cast<const uint32_t*>(x_dev); a.dtype = dtype; a.ld = ld; a.n = n; a.d = d; a.B = B; a.nbins = nbins_dev; a.edges = edges_dev;
    a.one_way = one_way_dev; a.two_way = two_way_dev; a.codes = static_cast<uint8_t*>(ws_dev);
    a.pairs = pairs; a.strips = (uint32_t)strips; a.rep = mg_replicas(B);
    hipLaunchKernelGGL(k_marginal_codes, dim3((unsigned)(row_blocks * col_blocks)), dim3(256), 0, s, a);
    int rc = check_launch(what);
    if (rc != D3P_OK || !pairs) return rc;
    hipLaunchKernelGGL(k_marginal_pairs, dim3((unsigned)(tiles * strips)), dim3(256), 0, s, a);
    return check_launch(what);
}

}  // extern "C"
