// CRPS and rank (PIT) counts of predictive draws against the observed outcomes (d3p_amd/scoring.py, include/d3p_hip.h):
// the entry d3p_col_crps with its host checks, and the two query functions.  The kernel k_col_crps<COLS>, its rule, its summation order
// and its LDS figures are in d3p_crps_kernel.h, which is compiled in d3p_hpdi.hip's translation unit: the kernel runs k_col_hpdi's
// staging and sort (d3p_colsort.h) on the order keys of d3p_colreduce.h, and the translation units that include that header are a
// fixed list.  This file therefore asks the HPDI entry's query functions for the forms and their limits, which are the same by
// construction, and reaches the kernel through col_crps_launch (d3p_crps.h).
#include "d3p_crps.h"

using namespace d3p;

extern "C" {

uint32_t d3p_col_crps_max_n(void) { return d3p_col_hpdi_max_n(); }

uint32_t d3p_col_crps_cols_per_group(uint32_t n) { return d3p_col_hpdi_cols_per_group(n); }

int d3p_col_crps(void* stream, const void* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t cols, const void* y_dev, float* out_dev,
                 int64_t out_ld, uint32_t* counts_dev, int64_t counts_ld)
{
    const char* what = "d3p_col_crps";
    if (!m_dev || !y_dev || !out_dev || !counts_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)m_dev | (uintptr_t)y_dev | (uintptr_t)out_dev | (uintptr_t)counts_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n >= 1 is required", what);
    if (ld < 0 || (uint64_t)ld < cols) return fail(D3P_E_INVALID_ARG, "%s: ld >= cols is required", what);
    if (out_ld < 0 || (uint64_t)out_ld < cols) return fail(D3P_E_INVALID_ARG, "%s: out_ld >= cols is required", what);
    if (counts_ld < 0 || (uint64_t)counts_ld < cols) return fail(D3P_E_INVALID_ARG, "%s: counts_ld >= cols is required", what);
    const uint32_t form = d3p_col_crps_cols_per_group(n);
    if (!form)
        return fail(D3P_E_UNSUPPORTED, "%s: n = %u draws; the column is sorted in LDS and n <= %u is served (there is no streamed form)", what, n,
                    d3p_col_crps_max_n());
    if (cols == 0) return D3P_OK;
    if (!is_device_ptr(m_dev) || !is_device_ptr(y_dev) || !is_device_ptr(out_dev) || !is_device_ptr(counts_dev))
        return fail(D3P_E_INVALID_ARG, "%s: the matrix, the observations and the outputs must be device memory", what);
    CrpsArgs a;
    a.m = static_cast<const uint32_t*>(m_dev); a.y = static_cast<const uint32_t*>(y_dev); a.dtype = dtype; a.ld = ld; a.n = n; a.cols = cols;
    a.out = out_dev; a.out_ld = out_ld; a.counts = counts_dev; a.counts_ld = counts_ld;
    return col_crps_launch(what, (hipStream_t)stream, a, form);
}

}  // extern "C"
