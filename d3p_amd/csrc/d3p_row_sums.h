// What the per-draw reductions over the ROWS of a table share, one definition each (DESIGN.md sections 4j, 4k, 4s, 4t):
//   d3p_loglik_draw_sums (d3p_draw_sums.hip)   d3p_rep_stats, d3p_predict_stats (d3p_rep_stats.hip)
//   d3p_predict_discrepancy (d3p_discrepancy.hip)   d3p_gmm_loglik_draw_sums (d3p_gmm_density.hip)
// The contract is a summation order that is a function of the arguments alone: the row tiles are cut into strips by row_strips, a
// workgroup walks the tiles of its strip ascending and writes its partials to the workspace as float64 [strip][K][n], and
// k_strip_merge adds the strips ascending from strip 0's.  No floating-point atomics.  The kernels that walk a strip stay their
// files' own; the regression family's (128-row tiles, D3P_ROW_SUMS_MAX_STRIPS) keep four quarter accumulators of 32 consecutive rows
// per tile and merge them with quarter_sum.  Measurements: docs/experiments_row_sums.md.
#pragma once
#include "d3p_device.h"
#include "d3p_host.h"

namespace d3p {

#define D3P_ROW_SUMS_MAX_STRIPS 512   // the regression entries' cap: they promise one another's order, so they share the constant

// THE strip function: tiles = ceil(rows / tile_rows); per = ceil(tiles / cap); strips = ceil(tiles / per) (<= cap) -- rows alone
// decide, not the device, its CU count or n
inline void row_strips(uint64_t rows, uint32_t tile_rows, uint32_t cap, uint32_t* tiles, uint32_t* per, uint32_t* strips)
{
    *tiles = cdiv(rows, tile_rows);
    *per = *tiles ? cdiv(*tiles, cap) : 0;
    *strips = *tiles ? cdiv(*tiles, *per) : 0;
}

// the [strip][K][n] float64 partials: refused with D3P_E_INVALID_ARG before any launch; sizer: the entry's *_workspace function
inline int row_workspace_check(const char* what, const char* sizer, const void* ws, size_t ws_bytes, uint32_t strips, uint32_t K, uint32_t n)
{
    const size_t need = (size_t)strips * K * n * sizeof(double);
    if (!ws || (uintptr_t)ws % sizeof(double)) return fail(D3P_E_INVALID_ARG, "%s: the workspace must be aligned to 8 bytes and not null", what);
    if (ws_bytes < need) return fail(D3P_E_INVALID_ARG, "%s: workspace of %zu bytes, %zu needed (%s)", what, ws_bytes, need, sizer);
    if (!is_device_ptr(ws)) return fail(D3P_E_INVALID_ARG, "%s: the workspace must be device memory", what);
    return D3P_OK;
}

// the tiles [t_lo, t_hi) of the workgroup's strip (grid x = strips)
__device__ __forceinline__ void strip_tiles(uint32_t per, uint32_t tiles, uint32_t& t_lo, uint32_t& t_hi)
{
    t_lo = blockIdx.x * per;
    t_hi = t_lo + per < tiles ? t_lo + per : tiles;
}

// the live rows among the lane's 32 rows r0 + col .. r0 + col + 31 of the tile at r0 (r0 < rows)
__device__ __forceinline__ int quarter_live_rows(uint64_t rows, uint64_t r0, int col)
{
    const uint64_t left = rows - r0;   // >= 1
    return left <= (uint64_t)col ? 0 : (left - col >= 32 ? 32 : (int)(left - col));
}

// one statistic's four quarters in the order q = 0, 1, 2, 3; r: [quarter][M draws] at the draw
__device__ __forceinline__ double quarter_sum(const double* r, int M)
{
#pragma clang fp contract(off)
    return ((r[0] + r[M]) + r[2 * M]) + r[3 * M];
}

// min / max by value with NaN carried: x NaN or m NaN gives NaN
__device__ __forceinline__ double rep_min(double m, double x) { return (m != m || x != x) ? m + x : (x < m ? x : m); }
__device__ __forceinline__ double rep_max(double m, double x) { return (m != m || x != x) ? m + x : (x > m ? x : m); }

// out[k n + s] = statistic k of draw s over the strips' partials part[strip][k][n] in ascending strip order, starting from strip 0's:
// a sum, or rep_min at k == MIN_AT and rep_max at k == MAX_AT (-1: none).  One thread per draw, grid ceil(n / 256).
template <int K, int MIN_AT, int MAX_AT>
__global__ void __launch_bounds__(256) k_strip_merge(const double* part, uint32_t strips, uint32_t n, double* out)
{
#pragma clang fp contract(off)
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    const double* p = part + s;
    double a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = p[k * (size_t)n];
    for (uint32_t t = 1; t < strips; ++t) {
        p += (size_t)K * n;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double x = p[k * (size_t)n];
            a[k] = k == MIN_AT ? rep_min(a[k], x) : k == MAX_AT ? rep_max(a[k], x) : a[k] + x;
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) out[k * (size_t)n + s] = a[k];
}

// the second launch of every entry above
template <int K, int MIN_AT, int MAX_AT>
inline int strip_merge(const char* what, hipStream_t s, const double* part, uint32_t strips, uint32_t n, double* out)
{
    hipLaunchKernelGGL((k_strip_merge<K, MIN_AT, MAX_AT>), dim3(cdiv(n, 256)), dim3(256), 0, s, part, strips, n, out);
    return check_launch(what);
}

}  // namespace d3p
