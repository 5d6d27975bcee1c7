// CRPS and rank (PIT) counts of predictive draws against the observed outcomes (d3p_amd/scoring.py, include/d3p_hip.h):
// the kernel of d3p_col_crps (the entry and its host checks: d3p_crps.hip).  This text is part of d3p_hpdi.hip's translation unit, the one
// of the reducers over a sorted column: it needs the order keys and the LDS opt-in of d3p_colreduce.h, and which translation units
// include that header is a fixed list (tests/test_colreduce_host.py), so d3p_hpdi.hip includes this file behind d3p_colreduce.h and
// d3p_colsort.h and nothing else does.  fp contract is off in that translation unit.  Per column c of a draws x cols matrix with n draws x_s and the observation y = y_c of the matrix's dtype, with the
// draws sorted ascending as s_0 <= .. <= s_{n-1} and d_i = (double)s_i - (double)y:
//   A = sum_i |d_i|                       G = sum_i (2 i - n + 1) d_i   (= 1/2 sum_i sum_j |x_i - x_j|: the pairwise form is never taken)
//   mae = A / n     spread = G / n^2     crps = A / n - G / n^2     crps_fair = A / n - G / (n (n - 1))
//   below = #{s : x_s < y}                equal = #{s : x_s == y}        (IEEE comparison: a NaN counts nowhere, -0 equals +0)
// n = 1: G = 0 and n (n - 1) = 0, so crps_fair = A - 0 / 0 = NaN: the 0 / 0 is the rule, not an accident.
//
// k_col_crps<COLS>: 256 threads, one workgroup owns COLS adjacent columns, thread t = (draw lane t / COLS, column lane t % COLS); the
// DL = 256 / COLS draw lanes of a column take the draws dl, dl + DL, ...  The forms and their limits over n are k_col_hpdi's
// (d3p_colsort.h): COLS = 32 (n <= 1152), 8 (n <= 4608), 2 (n <= 18432 = d3p_col_crps_max_n()).
//   pass 0   h_stage: every value once from memory, its key into dynamic LDS; per value the column's non-finite flag (a NaN or +-inf
//            draw; y is looked at once) and the two counts on the keys: key(x) < key(y), key(x) == key(y), NaNs excluded.  A lane
//            holds (below, equal, non-finite draws) as three 20-bit fields of ONE uint64 (each is at most n < 2^20); the column's
//            lanes merge by integer addition through LDS: order-independent.
//   sort     h_sort, in place on the keys.
//   scan     float64, fp contract off.  d_i = (double)s_i - (double)y is exact for int32 and rounds once for a float32 pair more than
//            29 binades apart; the coefficient 2 i - n + 1 is an exact integer cast; its product with d_i rounds once.
// Summation order (so that a column's bits are a function of its values, y and n alone): draw lane dl adds its terms i = dl, dl + DL,
// dl + 2 DL, .. in ascending i to a running A and a running G, both from +0; then the DL lanes of a column merge through static LDS in
// the fixed tree  r[dl] += r[dl + w]  for w = DL / 2, DL / 4, .. 1 (lane dl < w), the sum lying in lane 0.  DL is a function of the
// form, the form of n.  Each output is formed in float64 from A, G and n -- A / n, G / (n n), their difference -- and rounded to
// float32 once.  No floating-point atomics, no scratch, no workspace; a column past the end stands for n draws of 0 against y = 0 and
// writes nothing.  A column with the non-finite flag writes NaN in all four float rows; its counts are still the IEEE counts.
//
// Static LDS: 2 KiB of counts and 4 KiB of float64 sums, within the 9 KiB the reducers leave beside D3P_DYN_LDS_MAX.  The LDS bank
// picture of pass 0, the sort and the scan is k_col_hpdi's (d3p_hpdi.hip): the scan reads one key per draw, as its windows' lower ends.
#pragma once
#include "d3p_crps.h"

namespace d3p {

#define D3P_C_FIELD 20                // bits per count of a lane's packed word: n <= 18432 < 2^20

template <int COLS>
__global__ __launch_bounds__(256) void k_col_crps(CrpsArgs a)
{
    constexpr int DL = 256 / COLS;
    extern __shared__ __align__(16) unsigned char c_smem[];
    uint32_t* keys = reinterpret_cast<uint32_t*>(c_smem);   // [n][COLS]
    __shared__ uint64_t r_cnt[256];                         // [draw lane][column lane]: below | equal << 20 | non-finite << 40
    __shared__ double r_sum[2][256];                        // A and G

    const int t = threadIdx.x, cl = t & (COLS - 1), dl = t / COLS;
    const uint32_t n = a.n;
    const int32_t dtype = a.dtype;
    const uint64_t c = (uint64_t)blockIdx.x * COLS + cl;
    const bool live = c < a.cols;                           // a column past the end stands for n draws of 0 and writes nothing
    const uint32_t* col = a.m + (live ? c : 0);
    const uint32_t yw = live ? a.y[c] : 0u;
    const uint32_t ky = key_of(yw, dtype);
    const bool y_nan = !dtype && word_is_nan(yw);

    // pass 0: the keys, and per value the counts and the non-finite flag
    uint64_t cnt = 0ull;
    h_stage<COLS>(keys, col, (size_t)a.ld, live, cl, (uint32_t)dl, n, dtype, [&](uint32_t u, uint32_t k) {
        const bool ordered = !y_nan && (dtype || !word_is_nan(u));
        cnt += (uint64_t)(ordered && k < ky) | ((uint64_t)(ordered && k == ky) << D3P_C_FIELD)
               | ((uint64_t)(!dtype && !word_is_finite(u)) << (2 * D3P_C_FIELD));
    });
    r_cnt[t] = cnt;
    __syncthreads();
    for (int w = DL / 2; w > 0; w >>= 1) {
        if (dl < w) r_cnt[t] += r_cnt[t + w * COLS];
        __syncthreads();
    }
    cnt = r_cnt[cl];                                        // (r_cnt is not written again)

    h_sort<COLS>(keys, cl, (uint32_t)dl, n);

    // the scan: this lane's terms in ascending i
    const double y = dtype ? (double)(int32_t)yw : (double)__uint_as_float(yw);
    double A = 0.0, G = 0.0;
    for (uint32_t i = (uint32_t)dl; i < n; i += DL) {
        const uint32_t k = keys[(size_t)i * COLS + cl];
        const double d = (dtype ? (double)i32_of_key(k) : (double)f32_of_key(k)) - y;
        A += fabs(d);
        G += (double)(2 * (int64_t)i - (int64_t)n + 1) * d;
    }
    r_sum[0][t] = A;
    r_sum[1][t] = G;
    __syncthreads();
    for (int w = DL / 2; w > 0; w >>= 1) {
        if (dl < w) {
            r_sum[0][t] += r_sum[0][t + w * COLS];
            r_sum[1][t] += r_sum[1][t + w * COLS];
        }
        __syncthreads();
    }
    if (dl == 0 && live) {
        constexpr uint32_t MASK = (1u << D3P_C_FIELD) - 1u;
        const bool bad = (cnt >> (2 * D3P_C_FIELD)) != 0ull || (!dtype && !word_is_finite(yw));
        const double nn = (double)n;
        const double mae = r_sum[0][t] / nn;
        const double spread = r_sum[1][t] / (nn * nn);
        const double fair = r_sum[1][t] / (nn * (double)(n - 1u));   // n = 1: 0 / 0
        float* o = a.out + c;
        const size_t old = (size_t)a.out_ld;
        o[0] = bad ? NAN : (float)(mae - spread);
        o[old] = bad ? NAN : (float)(mae - fair);
        o[2 * old] = bad ? NAN : (float)mae;
        o[3 * old] = bad ? NAN : (float)spread;
        uint32_t* q = a.counts + c;
        q[0] = (uint32_t)cnt & MASK;
        q[(size_t)a.counts_ld] = (uint32_t)(cnt >> D3P_C_FIELD) & MASK;
    }
}

template <int COLS>
static int c_launch(const char* what, hipStream_t stream, const CrpsArgs& a)
{
    const uint64_t groups = (a.cols + COLS - 1) / COLS;
    if (groups > 0x7fffffffull) return fail(D3P_E_UNSUPPORTED, "%s: cols <= %d (2^31 - 1) at n = %u", what, COLS, a.n);
    const size_t lds = (size_t)COLS * a.n * 4;
    if (lds > 48u * 1024u)
        if (int rc = dynamic_lds_opt_in(reinterpret_cast<const void*>(&k_col_crps<COLS>), D3P_DYN_LDS_MAX, what)) return rc;
    hipLaunchKernelGGL((k_col_crps<COLS>), dim3((unsigned)groups), dim3(256), lds, stream, a);
    return check_launch(what);
}

// what d3p_crps.hip calls after its host checks: `form` = h_cols_per_group(a.n), not 0
int col_crps_launch(const char* what, hipStream_t stream, const CrpsArgs& a, uint32_t form)
{
    if (form == 32u) return c_launch<32>(what, stream, a);
    if (form == 8u) return c_launch<8>(what, stream, a);
    return c_launch<2>(what, stream, a);
}

}  // namespace d3p
