// What d3p_crps.hip (the entry d3p_col_crps and its host checks) and d3p_crps_kernel.h (k_col_crps, compiled in d3p_hpdi.hip's
// translation unit beside the sort and the order keys it uses) share: the launch arguments and the launch itself.
#pragma once
#include "d3p_host.h"

namespace d3p {

struct CrpsArgs {
    const uint32_t* m;   // the matrix's words: float32 or int32
    const uint32_t* y;   // cols words of the same dtype
    int32_t dtype;       // 0: float32, 1: int32
    int64_t ld;
    uint32_t n;
    uint64_t cols;
    float* out;          // 4 rows: crps, crps_fair, mae, spread
    int64_t out_ld;
    uint32_t* counts;    // 2 rows: below, equal
    int64_t counts_ld;
};

// launches k_col_crps<form>; `form` = d3p_col_crps_cols_per_group(a.n), not 0 (d3p_crps_kernel.h)
int col_crps_launch(const char* what, hipStream_t stream, const CrpsArgs& a, uint32_t form);

}  // namespace d3p
