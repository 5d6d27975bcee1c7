// What d3p_sort_columns.hip (the entries d3p_sort_columns and d3p_column_cdf_distance, their host checks and query functions) and
// d3p_colsort_global_kernel.h (the kernels, compiled in d3p_quantiles.hip's translation unit beside the order keys they use) share: the
// geometry, the launch arguments and the launches themselves.
#pragma once
#include "d3p_host.h"

namespace d3p {

#define D3P_CS_T 4096u              // a block: consecutive positions of one column per workgroup (256 threads x 16 keys)
#define D3P_CS_STAGE 8192u          // sorted keys staged in LDS by the two-level search (32 KiB)
#define D3P_CS_RANK_STRIP 16384u    // positions of one column per workgroup of k_cs_ranks: one staging serves four blocks
#define D3P_CS_THREAD_KEYS 16u      // keys (positions) a thread owns in a block: the length of its float64 chain in k_cdf_part

struct CsArgs {
    const uint32_t* x;   // the table's words: float32 or int32, row-major
    int32_t dtype;       // 0: float32, 1: int32
    int64_t ld;
    uint32_t n, d;
    uint32_t* out;       // d x ld_s: keys after the second pass, the stored words after the fourth
    int64_t ld_s;
    int32_t* ranks2;     // n x ld_r, or null
    int64_t ld_r;
    uint32_t* w0;        // d x n: the unsorted keys, column-major
    uint32_t* w1;        // d x n: the other key buffer; at the end the doubled midranks, column-major
    uint32_t* hist;      // d x 256 x nblk: per column the block counts of a digit, digit-major; scanned in place
    uint32_t nblk;       // ceil(n / D3P_CS_T)
};

struct CdfArgs {
    const uint32_t* a;   // d x ld_a sorted stored words
    const uint32_t* b;   // d x ld_b
    int64_t ld_a, ld_b;
    uint32_t n_a, n_b, d;
    int32_t dtype;
    uint32_t nblk_a, nblk_b;
    double* part_w1;     // d x (nblk_a + nblk_b) each: a block's float64 partial, its largest numerator and the smallest key that attains it
    uint64_t* part_num;
    uint32_t* part_key;
    uint64_t* ks_num;    // d each
    uint32_t* ks_at;
    double* w1;
};

inline uint32_t cs_blocks(uint64_t n) { return (uint32_t)((n + D3P_CS_T - 1u) / D3P_CS_T); }
// S: every S-th key of a sorted column of n is staged, at most D3P_CS_STAGE of them
inline uint32_t cs_stride(uint64_t n) { return (uint32_t)((n + D3P_CS_STAGE - 1u) / D3P_CS_STAGE); }

int cs_sort_launch(const char* what, hipStream_t stream, const CsArgs& a);
int cs_cdf_launch(const char* what, hipStream_t stream, const CdfArgs& a);

}  // namespace d3p
