// Column sorts for any n, the doubled midranks behind them and the KS / Wasserstein-1 distances of two sorted tables
// (d3p_amd/univariate.py, include/d3p_hip.h): the entries d3p_sort_columns and d3p_column_cdf_distance with their host
// checks, and the query functions.  The kernels, their rule, their summation order and their LDS figures are in
// d3p_colsort_global_kernel.h, which is compiled in d3p_quantiles.hip's translation unit: they work on the order keys of the column
// reducers, and the translation units that include that header are a fixed list.  This file reaches them through cs_sort_launch and
// cs_cdf_launch (d3p_sort_columns.h), names no key map and opts into nothing: every kernel has static LDS below 48 KiB.
#include "d3p_sort_columns.h"

using namespace d3p;

namespace {

const uint64_t CS_MAX_N = 0x7fffffffull;   // 2^31 - 1
const uint64_t CS_MAX_GROUPS = 0x7fffffffull;

bool cs_mul_fits(uint64_t a, uint64_t b) { return b == 0 || a <= (uint64_t)INT64_MAX / b; }

// the workgroups of the largest grid of a sort: d x blocks (the tiles of the two transposes are fewer)
uint64_t cs_sort_groups(uint64_t n, uint32_t d) { return (uint64_t)d * cs_blocks(n); }

size_t cs_sort_workspace(uint64_t n, uint32_t d)
{
    if (n < 1 || n > CS_MAX_N || d < 1) return 0;
    if (cs_sort_groups(n, d) > CS_MAX_GROUPS) return 0;
    const uint64_t words = 2u * n * d + 256ull * cs_blocks(n) * d;   // (n d < 2^43 here: d x blocks fits 31 bits)
    return (size_t)(4u * words);
}

size_t cs_cdf_workspace(uint64_t n_a, uint64_t n_b, uint32_t d)
{
    if (n_a < 1 || n_a > CS_MAX_N || n_b < 1 || n_b > CS_MAX_N || d < 1) return 0;
    const uint64_t parts = (uint64_t)d * ((uint64_t)cs_blocks(n_a) + cs_blocks(n_b));
    if (parts > CS_MAX_GROUPS) return 0;
    return (size_t)(parts * 20u + 4u) & ~(size_t)7u;   // 8 + 8 + 4 bytes per (column, block), rounded to 8
}

}  // namespace

extern "C" {

uint32_t d3p_sort_columns_block_keys(void) { return D3P_CS_T; }

uint32_t d3p_sort_columns_staged_keys(void) { return D3P_CS_STAGE; }

uint32_t d3p_sort_columns_rank_stride(uint64_t n) { return n < 1 || n > CS_MAX_N ? 0u : cs_stride(n); }

size_t d3p_sort_columns_workspace(uint64_t n, uint32_t d, int32_t want_ranks)
{
    if (want_ranks != 0 && want_ranks != 1) return 0;
    if (want_ranks && n > (CS_MAX_N >> 1)) return 0;
    return cs_sort_workspace(n, d);   // (the midranks pass through the second key buffer, which is free by then)
}

int d3p_sort_columns(void* stream, const void* x_dev, int32_t dtype, int64_t ld, uint64_t n, uint32_t d, void* sorted_dev, int64_t ld_s,
                     int32_t* ranks2_dev, int64_t ld_r, void* ws_dev, size_t ws_bytes)
{
    const char* what = "d3p_sort_columns";
    if (!x_dev || !sorted_dev || !ws_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)x_dev | (uintptr_t)sorted_dev | (uintptr_t)ranks2_dev | (uintptr_t)ws_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (n < 1 || n > CS_MAX_N) return fail(D3P_E_INVALID_ARG, "%s: 1 <= n <= 2^31 - 1 rows are required", what);
    if (ranks2_dev && n > (CS_MAX_N >> 1))
        return fail(D3P_E_INVALID_ARG, "%s: the doubled midranks are int32: n <= 2^30 - 1 rows with ranks2_dev", what);
    if (d < 1) return fail(D3P_E_INVALID_ARG, "%s: d >= 1 is required", what);
    if (ld < 0 || (uint64_t)ld < d) return fail(D3P_E_INVALID_ARG, "%s: ld >= d is required", what);
    if (ld_s < 0 || (uint64_t)ld_s < n) return fail(D3P_E_INVALID_ARG, "%s: ld_s >= n is required", what);
    if (ranks2_dev && (ld_r < 0 || (uint64_t)ld_r < d)) return fail(D3P_E_INVALID_ARG, "%s: ld_r >= d is required", what);
    if (!cs_mul_fits(n, (uint64_t)ld) || !cs_mul_fits(d, (uint64_t)ld_s) || (ranks2_dev && !cs_mul_fits(n, (uint64_t)ld_r)))
        return fail(D3P_E_INVALID_ARG, "%s: n * ld, d * ld_s or n * ld_r does not fit 63 bits", what);
    const uint64_t groups = cs_sort_groups(n, d);
    if (groups > CS_MAX_GROUPS)
        return fail(D3P_E_UNSUPPORTED, "%s: %u columns x %u blocks of rows = %llu workgroups, more than 2^31 - 1", what, d, cs_blocks(n),
                    (unsigned long long)groups);
    const size_t need = cs_sort_workspace(n, d);
    if (ws_bytes < need) return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_bytes, need);
    if (!is_device_ptr(x_dev) || !is_device_ptr(sorted_dev) || !is_device_ptr(ws_dev) || (ranks2_dev && !is_device_ptr(ranks2_dev)))
        return fail(D3P_E_INVALID_ARG, "%s: the table, the outputs and the workspace must be device memory", what);
    CsArgs a;
    a.x = static_cast<const uint32_t*>(x_dev); a.dtype = dtype; a.ld = ld; a.n = (uint32_t)n; a.d = d;
    a.out = static_cast<uint32_t*>(sorted_dev); a.ld_s = ld_s; a.ranks2 = ranks2_dev; a.ld_r = ld_r;
    a.nblk = cs_blocks(n);
    a.w0 = static_cast<uint32_t*>(ws_dev);
    a.w1 = a.w0 + (size_t)n * d;
    a.hist = a.w1 + (size_t)n * d;
    return cs_sort_launch(what, (hipStream_t)stream, a);
}

size_t d3p_column_cdf_distance_workspace(uint64_t n_a, uint64_t n_b, uint32_t d) { return cs_cdf_workspace(n_a, n_b, d); }

uint32_t d3p_column_cdf_distance_roundings(uint64_t n_a, uint64_t n_b)
{
    if (n_a < 1 || n_a > CS_MAX_N || n_b < 1 || n_b > CS_MAX_N) return 0u;
    return 5u + D3P_CS_THREAD_KEYS + 8u + cs_blocks(n_a) + cs_blocks(n_b);   // a term; a thread's chain; the tree of 256; the merge
}

int d3p_column_cdf_distance(void* stream, const void* a_dev, int64_t ld_a, uint64_t n_a, const void* b_dev, int64_t ld_b, uint64_t n_b,
                            int32_t dtype, uint32_t d, uint64_t* ks_num_dev, void* ks_at_dev, double* w1_dev, void* ws_dev, size_t ws_bytes)
{
    const char* what = "d3p_column_cdf_distance";
    if (!a_dev || !b_dev || !ks_num_dev || !ks_at_dev || !w1_dev || !ws_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)a_dev | (uintptr_t)b_dev | (uintptr_t)ks_at_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a_dev, b_dev or ks_at_dev is not aligned to 4 bytes", what);
    if ((((uintptr_t)ks_num_dev | (uintptr_t)w1_dev | (uintptr_t)ws_dev) & 7u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: ks_num_dev, w1_dev or ws_dev is not aligned to 8 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (n_a < 1 || n_a > CS_MAX_N || n_b < 1 || n_b > CS_MAX_N)
        return fail(D3P_E_INVALID_ARG, "%s: 1 <= n_a, n_b <= 2^31 - 1 are required (n_a n_b < 2^63)", what);
    if (d < 1) return fail(D3P_E_INVALID_ARG, "%s: d >= 1 is required", what);
    if (ld_a < 0 || (uint64_t)ld_a < n_a || ld_b < 0 || (uint64_t)ld_b < n_b)
        return fail(D3P_E_INVALID_ARG, "%s: ld_a >= n_a and ld_b >= n_b are required", what);
    if (!cs_mul_fits(d, (uint64_t)ld_a) || !cs_mul_fits(d, (uint64_t)ld_b))
        return fail(D3P_E_INVALID_ARG, "%s: d * ld_a or d * ld_b does not fit 63 bits", what);
    const uint32_t nblk_a = cs_blocks(n_a), nblk_b = cs_blocks(n_b);
    const uint64_t parts = (uint64_t)d * ((uint64_t)nblk_a + nblk_b);
    if (parts > CS_MAX_GROUPS)
        return fail(D3P_E_UNSUPPORTED, "%s: %u columns x %u blocks of positions = %llu workgroups, more than 2^31 - 1", what, d, nblk_a + nblk_b,
                    (unsigned long long)parts);
    const size_t need = cs_cdf_workspace(n_a, n_b, d);
    if (ws_bytes < need) return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_bytes, need);
    if (!is_device_ptr(a_dev) || !is_device_ptr(b_dev) || !is_device_ptr(ks_num_dev) || !is_device_ptr(ks_at_dev) || !is_device_ptr(w1_dev) ||
        !is_device_ptr(ws_dev))
        return fail(D3P_E_INVALID_ARG, "%s: the tables, the outputs and the workspace must be device memory", what);
    CdfArgs g;
    g.a = static_cast<const uint32_t*>(a_dev); g.b = static_cast<const uint32_t*>(b_dev); g.ld_a = ld_a; g.ld_b = ld_b;
    g.n_a = (uint32_t)n_a; g.n_b = (uint32_t)n_b; g.d = d; g.dtype = dtype; g.nblk_a = nblk_a; g.nblk_b = nblk_b;
    g.part_w1 = static_cast<double*>(ws_dev);
    g.part_num = reinterpret_cast<uint64_t*>(g.part_w1 + parts);
    g.part_key = reinterpret_cast<uint32_t*>(g.part_num + parts);
    g.ks_num = ks_num_dev; g.ks_at = static_cast<uint32_t*>(ks_at_dev); g.w1 = w1_dev;
    return cs_cdf_launch(what, (hipStream_t)stream, g);
}

}  // extern "C"
