// The in-LDS column sort that the reducers which need a WHOLE sorted column share: k_col_hpdi (d3p_hpdi.hip) and k_col_crps (d3p_crps_kernel.h).
// Device only.  256 threads, one workgroup owns COLS adjacent columns, thread t = (draw lane t / COLS, column lane t % COLS); the keys
// (key_of, d3p_colreduce.h) lie in dynamic LDS as [draw][COLS].
//   h_stage  pass 0: every value once from memory, D3P_H_ILP loads in flight per thread, its key into LDS; the caller's `each(word,
//            key)` sees every value of the thread's draws (a NaN flag, counts).
//   h_sort   a bitonic network in its all-ascending form, in place on the keys: per size k = 2, 4, .. one "flip" step (i against the
//            mirror position of its block of k) and then the steps at distance k/4, k/8, .. 1 (i against i + j).  Every
//            compare-exchange puts the smaller key at the lower index, so positions >= n behave as keys above all others that never
//            move: a compare-exchange whose partner is >= n is skipped and n needs no padding to a power of two.  One barrier per
//            step; within a step a thread loads the keys of eight of its pairs before it stores any (the pairs are disjoint).
// The forms differ only in COLS: 32 (n <= 1152), 8 (n <= 4608), 2 (n <= 18432): 4 n COLS bytes of keys within D3P_DYN_LDS_MAX; the
// widest form that fits is taken (h_cols_per_group).  A new reducer over sorted columns uses this header and defines no network,
// no staging and no form rule of its own.  The header builds on d3p_colreduce.h (key_of, D3P_DYN_LDS_MAX) and is included BEHIND it by
// the one translation unit of the sorted-column reducers, d3p_hpdi.hip, which also compiles d3p_crps_kernel.h: which translation units
// include d3p_colreduce.h is a fixed list (tests/test_colreduce_host.py), and this header does not add itself to it.
#pragma once

namespace d3p {

#define D3P_H_ILP 8                   // pairs of a network step, and loads of pass 0, a thread has in flight
#define D3P_H_MAX_N(COLS) (D3P_DYN_LDS_MAX / (4 * (COLS)))   // 1152 | 4608 | 18432

// columns per workgroup at n draws: 32 | 8 | 2, or 0 where the column does not fit the LDS (host)
inline uint32_t h_cols_per_group(uint32_t n)
{
    if (n < 1 || n > (uint32_t)D3P_H_MAX_N(2)) return 0u;
    return n <= (uint32_t)D3P_H_MAX_N(32) ? 32u : n <= (uint32_t)D3P_H_MAX_N(8) ? 8u : 2u;
}

// One step of the network on the keys [n][COLS] of column lane cl, the pairs dl, dl + DL, .. of the step:
//   FLIP   lg = log2 k:  pair p of block p / (k/2) is (block k + off, block k + k - 1 - off), off = p mod (k/2)
//   else   lg = log2 j:  pair p is (i, i + j), i = (p / j) 2 j + p mod j
// The indices rise with p, so the pairs whose lower index (FLIP) or both indices (else) lie below n are a prefix 0 .. cnt - 1; a flip
// pair whose upper index is >= n is skipped.  The pairs of a step are disjoint: a thread loads the keys of D3P_H_ILP of its pairs
// before it stores any, which keeps that many LDS loads in flight where the keys fill the LDS and one wave runs per SIMD.
template <int COLS, bool FLIP>
__device__ inline void h_step(uint32_t* keys, int cl, uint32_t dl, uint32_t n, uint32_t lg)
{
    constexpr uint32_t DL = 256 / COLS;
    const uint32_t w = 1u << lg;   // FLIP: k, else: j
    uint32_t cnt;
    if (FLIP) {
        const uint32_t h = w >> 1, r = n & (w - 1u);
        cnt = (n >> lg) * h + (r < h ? r : h);
    } else {
        const uint32_t r = n & (2u * w - 1u);
        cnt = (n >> (lg + 1)) * w + (r > w ? r - w : 0u);
    }
    for (uint32_t p0 = dl; p0 < cnt; p0 += D3P_H_ILP * DL) {
        uint32_t ia[D3P_H_ILP], ib[D3P_H_ILP], ka[D3P_H_ILP], kb[D3P_H_ILP];
        bool ok[D3P_H_ILP];
#pragma unroll
        for (int u = 0; u < D3P_H_ILP; ++u) {
            const uint32_t p = p0 + (uint32_t)u * DL;
            if (FLIP) {
                const uint32_t base = (p >> (lg - 1)) << lg, off = p & ((w >> 1) - 1u);
                ia[u] = base + off;
                ib[u] = base + w - 1u - off;
                ok[u] = p < cnt && ib[u] < n;
            } else {
                ia[u] = ((p >> lg) << (lg + 1)) + (p & (w - 1u));
                ib[u] = ia[u] + w;
                ok[u] = p < cnt;
            }
            ka[u] = kb[u] = 0u;
            if (ok[u]) {
                ka[u] = keys[(size_t)ia[u] * COLS + cl];
                kb[u] = keys[(size_t)ib[u] * COLS + cl];
            }
        }
#pragma unroll
        for (int u = 0; u < D3P_H_ILP; ++u) {
            if (ok[u] && ka[u] > kb[u]) {
                keys[(size_t)ia[u] * COLS + cl] = kb[u];
                keys[(size_t)ib[u] * COLS + cl] = ka[u];
            }
        }
    }
}

// pass 0: the keys of the draws dl, dl + DL, .. of the column `col` (leading dimension ld; a column that is not live stands for n
// draws of 0) into LDS; each(word, key) per value.  No barrier: the caller's first one follows.
template <int COLS, class Each>
__device__ inline void h_stage(uint32_t* keys, const uint32_t* col, size_t ld, bool live, int cl, uint32_t dl, uint32_t n, int32_t dtype, Each each)
{
    constexpr uint32_t DL = 256 / COLS;
    for (uint32_t s0 = dl; s0 < n; s0 += D3P_H_ILP * DL) {
        uint32_t u[D3P_H_ILP];
#pragma unroll
        for (int q = 0; q < D3P_H_ILP; ++q) {
            const uint32_t s = s0 + (uint32_t)q * DL;
            u[q] = live && s < n ? col[(size_t)s * ld] : 0u;
        }
#pragma unroll
        for (int q = 0; q < D3P_H_ILP; ++q) {
            const uint32_t s = s0 + (uint32_t)q * DL;
            if (s < n) {
                const uint32_t k = key_of(u[q], dtype);
                each(u[q], k);
                keys[(size_t)s * COLS + cl] = k;
            }
        }
    }
}

// the sort: sizes k = 2^lk while k / 2 < n (positions >= n never move: a partner there is skipped).  Every thread of the workgroup
// calls it after a barrier behind the last store of a key; every step ends in a barrier (n = 1 has no step: the caller's barrier stands).
template <int COLS>
__device__ inline void h_sort(uint32_t* keys, int cl, uint32_t dl, uint32_t n)
{
    for (uint32_t lk = 1; (1u << (lk - 1)) < n; ++lk) {
        h_step<COLS, true>(keys, cl, dl, n, lk);            // flip within blocks of k = 2^lk
        __syncthreads();
        for (uint32_t lj = lk - 1; lj-- > 0;) {             // distance 2^lj = k / 4 .. 1
            h_step<COLS, false>(keys, cl, dl, n, lj);
            __syncthreads();
        }
    }
}

}  // namespace d3p
