// Highest-density intervals (d3p_amd/intervals.py, include/d3p_hip.h): numpyro.diagnostics.hpdi per column of a
// draws x cols matrix, d3p_col_hpdi.  Per column of n draws and per window length L (computed by the host as int(prob n)):
//   s = the draws sorted ascending;  len[i] = s[i + L] - s[i], i = 0 .. n - L - 1;  i* = the first minimum of len (a NaN length is
//   below every other, np.argmin's rule);  the interval is (s[i*], s[i* + L]).
// Unlike d3p_col_quantiles, which selects two order statistics, this needs the whole sorted column: the column is sorted in LDS.
//
// k_col_hpdi<COLS>: 256 threads, one workgroup owns COLS adjacent columns, thread t = (draw lane t / COLS, column lane t % COLS); the
// DL = 256 / COLS draw lanes of a column take the draws (pairs, windows) dl, dl + DL, ...
//   pass 0   every value once from memory, eight loads in flight per thread: the column's NaN flag, and its order-preserving uint32
//            key (key_of, d3p_colreduce.h) into dynamic LDS as [draw][COLS] (h_stage, d3p_colsort.h).
//   sort     the shared bitonic network (h_sort, d3p_colsort.h), in place on the keys.
//   scan     per L one pass over the n - L windows: each draw lane keeps the minimum of (length, i) as ONE uint64 = rank(length) << 32
//            | i, the column's lanes merge theirs through LDS (a tree of minima: order-independent, so the bits are a function of the
//            column's values and (n, L) alone).  rank: float32 lengths are >= +0, +inf or NaN (inf - inf): NaN -> 0, else the bits
//            + 1; int32 lengths are the exact difference of the keys, at most 2^32 - 1.
// The forms differ only in COLS: 32 (n <= 1152), 8 (n <= 4608), 2 (n <= 18432 = d3p_col_hpdi_max_n()): 4 n COLS bytes of keys within
// the 144 KiB of dynamic LDS that k_col_quantiles and k_psis_loo use; the widest form that fits is taken.  No streamed form.
// No floating-point atomics, no scratch, no workspace; a column past the end stands for n draws of 0 and writes nothing.
//
// LDS banks: every access is a 4-byte load or store, served in lane groups of 32 over 32 banks.  A group holds G = 32 /
// COLS draw lanes with consecutive pair (window) numbers.  COLS = 32: a group is one draw's 32 consecutive words, no conflict at any
// step.  COLS = 8 (G = 4) and COLS = 2 (G = 16): the bank is (index mod G) COLS + column lane; at a distance j >= G the G lower (upper)
// indices of a group are consecutive, no conflict; at j < G they are runs of j with gaps of j, which fall two by two on the same
// banks: a 2-way conflict on the loads of those steps (the last log2(G) steps of every size), none in pass 0 or the scan.
#include "d3p_colreduce.h"
#include "d3p_colsort.h"
#include "d3p_device.h"

#pragma clang fp contract(off)

namespace d3p {

#define D3P_H_MAX 8                   // window lengths per launch

struct HpdiArgs {
    const uint32_t* m;   // the matrix's words: float32 or int32
    int32_t dtype;       // 0: float32, 1: int32
    int64_t ld;
    uint32_t n;
    uint64_t cols;
    uint32_t Q;
    uint32_t len[D3P_H_MAX];
    float* out;
    int64_t out_ld;
};

// the stored value of a key as float32: exact for float32, one rounding for an int32 count above 2^24
__device__ inline float h_value(uint32_t k, int32_t dtype) { return dtype ? (float)i32_of_key(k) : f32_of_key(k); }

// rank(length of the window lo .. hi) << 32 | i: smaller is better, a NaN length is lowest
__device__ inline uint64_t h_window(uint32_t klo, uint32_t khi, uint32_t i, int32_t dtype)
{
    uint32_t r;
    if (dtype) {
        r = khi - klo;                                     // the exact difference: the keys are the values + 2^31
    } else {
        const float d = h_value(khi, 0) - h_value(klo, 0);   // one rounding (fp contract is off): >= +0, +inf, or NaN from inf - inf
        r = d != d ? 0u : __float_as_uint(d) + 1u;
    }
    return ((uint64_t)r << 32) | i;
}

template <int COLS>
__global__ __launch_bounds__(256) void k_col_hpdi(HpdiArgs a)
{
    constexpr int DL = 256 / COLS;
    extern __shared__ __align__(16) unsigned char h_smem[];
    uint32_t* keys = reinterpret_cast<uint32_t*>(h_smem);   // [n][COLS]
    __shared__ uint64_t r_min[256];                         // [draw lane][column lane]

    const int t = threadIdx.x, cl = t & (COLS - 1), dl = t / COLS;
    const uint32_t n = a.n;
    const int32_t dtype = a.dtype;
    const uint64_t c = (uint64_t)blockIdx.x * COLS + cl;
    const bool live = c < a.cols;                           // a column past the end stands for n draws of 0 and writes nothing
    const uint32_t* col = a.m + (live ? c : 0);
    const size_t ld = (size_t)a.ld;
#define H_KEY(s) keys[(size_t)(s) * COLS + cl]

    // pass 0: the column's NaN flag and its keys; D3P_H_ILP loads from memory in flight per thread
    uint32_t nan = 0u;
    h_stage<COLS>(keys, col, ld, live, cl, (uint32_t)dl, n, dtype, [&](uint32_t u, uint32_t) {
        if (!dtype && word_is_nan(u)) nan = 1u;
    });
    r_min[t] = nan;
    __syncthreads();
    for (int w = DL / 2; w > 0; w >>= 1) {
        if (dl < w) r_min[t] |= r_min[t + w * COLS];
        __syncthreads();
    }
    nan = (uint32_t)r_min[cl];
    __syncthreads();

    h_sort<COLS>(keys, cl, (uint32_t)dl, n);

    for (uint32_t qi = 0; qi < a.Q; ++qi) {
        const uint32_t L = a.len[qi];                       // L <= n - 1: at least one window
        uint64_t best = ~0ull;
        for (uint32_t i = dl; i + L < n; i += DL) {
            const uint64_t w = h_window(H_KEY(i), H_KEY(i + L), i, dtype);
            best = w < best ? w : best;
        }
        r_min[t] = best;
        __syncthreads();
        for (int w = DL / 2; w > 0; w >>= 1) {
            if (dl < w) {
                const uint64_t o = r_min[t + w * COLS];
                if (o < r_min[t]) r_min[t] = o;
            }
            __syncthreads();
        }
        if (dl == 0 && live) {
            const uint32_t i = (uint32_t)r_min[t];
            float* o = a.out + (size_t)(2u * qi) * (size_t)a.out_ld + c;
            o[0] = nan ? NAN : h_value(H_KEY(i), dtype);
            o[(size_t)a.out_ld] = nan ? NAN : h_value(H_KEY(i + L), dtype);
        }
        __syncthreads();   // (r_min is free for the next length)
    }
#undef H_KEY
}

template <int COLS>
static int h_launch(const char* what, hipStream_t stream, const HpdiArgs& a)
{
    const uint64_t groups = (a.cols + COLS - 1) / COLS;
    if (groups > 0x7fffffffull) return fail(D3P_E_UNSUPPORTED, "%s: cols <= %d (2^31 - 1) at n = %u", what, COLS, a.n);
    const size_t lds = (size_t)COLS * a.n * 4;
    if (lds > 48u * 1024u)
        if (int rc = dynamic_lds_opt_in(reinterpret_cast<const void*>(&k_col_hpdi<COLS>), D3P_DYN_LDS_MAX, what)) return rc;
    hipLaunchKernelGGL((k_col_hpdi<COLS>), dim3((unsigned)groups), dim3(256), lds, stream, a);
    return check_launch(what);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_col_hpdi_max_n(void) { return (uint32_t)D3P_H_MAX_N(2); }

uint32_t d3p_col_hpdi_cols_per_group(uint32_t n)
{
    return h_cols_per_group(n);
}

int d3p_col_hpdi(void* stream, const void* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t cols, uint32_t Q, const uint32_t* len_host,
                 float* out_dev, int64_t out_ld)
{
    const char* what = "d3p_col_hpdi";
    if (!m_dev || !out_dev || !len_host) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if (!aligned4(m_dev) || !aligned4(out_dev)) return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n >= 1 is required", what);
    if (Q < 1 || Q > D3P_H_MAX) return fail(D3P_E_INVALID_ARG, "%s: 1 <= Q <= 8 (Q = %u)", what, Q);
    if (is_device_ptr(len_host)) return fail(D3P_E_INVALID_ARG, "%s: len_host must be host memory", what);
    HpdiArgs a;
    for (uint32_t q = 0; q < Q; ++q) {
        if (len_host[q] >= n) return fail(D3P_E_INVALID_ARG, "%s: len[%u] = %u is not below n = %u", what, q, len_host[q], n);
        a.len[q] = len_host[q];
    }
    for (uint32_t q = Q; q < D3P_H_MAX; ++q) a.len[q] = 0u;
    if (ld < 0 || (uint64_t)ld < cols) return fail(D3P_E_INVALID_ARG, "%s: ld >= cols is required", what);
    if (out_ld < 0 || (uint64_t)out_ld < cols) return fail(D3P_E_INVALID_ARG, "%s: out_ld >= cols is required", what);
    const uint32_t form = d3p_col_hpdi_cols_per_group(n);
    if (!form)
        return fail(D3P_E_UNSUPPORTED, "%s: n = %u draws; the column is sorted in LDS and n <= %u is served (there is no streamed form)", what, n,
                    d3p_col_hpdi_max_n());
    if (cols == 0) return D3P_OK;
    if (!is_device_ptr(m_dev) || !is_device_ptr(out_dev)) return fail(D3P_E_INVALID_ARG, "%s: the matrix and the output must be device memory", what);
    a.m = static_cast<const uint32_t*>(m_dev); a.dtype = dtype; a.ld = ld; a.n = n; a.cols = cols; a.Q = Q; a.out = out_dev; a.out_ld = out_ld;
    if (form == 32u) return h_launch<32>(what, (hipStream_t)stream, a);
    if (form == 8u) return h_launch<8>(what, (hipStream_t)stream, a);
    return h_launch<2>(what, (hipStream_t)stream, a);
}

}  // extern "C"

// k_col_crps, the second reducer over a sorted column, is compiled here: it shares the sort above and the keys of d3p_colreduce.h
#include "d3p_crps_kernel.h"
