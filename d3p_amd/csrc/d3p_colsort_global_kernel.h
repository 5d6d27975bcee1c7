// Every column of a table sorted over ALL its rows, the doubled midranks behind the sort, and the KS / Wasserstein-1 distances of two
// sorted tables (d3p_amd/univariate.py, include/d3p_hip.h): the kernels of d3p_sort_columns and d3p_column_cdf_distance
// (the entries and their host checks: d3p_sort_columns.hip).  This text is part of d3p_quantiles.hip's translation unit: it needs the
// order keys of d3p_colreduce.h, and which translation units include that header is a fixed list (tests/test_colreduce_host.py), so
// d3p_quantiles.hip includes this file behind d3p_colreduce.h and nothing else does.  fp contract is off in that translation unit.
//
// THE SORT is a least-significant-digit radix sort on the uint32 order keys (key_of), 8-bit digits, four passes, keys only, segmented:
// every launch serves all d columns.  A block is D3P_CS_T = 4096 consecutive positions of one column and one workgroup of 256 threads;
// every grid is one-dimensional, workgroup g = (column g / nblk, block g % nblk).
//   k_cs_keys      tiles of 64 rows x 64 columns of the row-major table: a wavefront reads 256 contiguous bytes of a row, the tile goes
//                  through LDS ([64][65] words: the transposed read walks a stride of 65 words, 64 lanes on 32 banks twice, no further
//                  conflict) and the KEYS are written column-major to W0, a wavefront 256 contiguous bytes of a column.
//   per pass p = 0 .. 3, source and destination W0 -> W1 -> out -> W1 -> out:
//   k_cs_hist      per (column, block) the 256 counts of digit p: integer LDS atomics on one histogram per wavefront, summed, written
//                  digit-major (hist[column][digit][block]).
//   k_cs_scan      one workgroup per column, thread t = digit t: the exclusive scan over (digit, block) in digit-major order, which is
//                  the flat order of the column's counts: a thread sums its run of nblk counts, one block scan of the 256 sums, the
//                  thread rewrites its run.  No workgroup waits for another.
//   k_cs_scatter   STABLE.  A wavefront owns 1024 consecutive keys and takes them in 16 rounds of 64 consecutive keys.  A lane's rank
//                  among the lanes of its round with its digit: eight ballots build the match mask bit by bit, rank = popcount(mask &
//                  lanes below).  Per wavefront and digit a running count in LDS: every lane reads it, the lowest matching lane adds the
//                  round's matches.  After a barrier thread t = digit t turns the four wavefronts' counts into the block's digit starts
//                  (one block scan) and each wavefront's offset; the keys are placed in digit order in 16 KiB of LDS and written out:
//                  key i of the block goes to (scanned base of its digit) + (i - the digit's start), so consecutive lanes write
//                  consecutive addresses inside a digit run.  The fourth pass writes the stored words (f32_of_key / i32_of_key: -0
//                  comes out as +0, negative NaNs first, positive NaNs last).
// W0 still holds the unsorted keys afterwards.  THE RANKS (k_cs_ranks, a column and a strip of D3P_CS_RANK_STRIP positions per
// workgroup): every S-th key of the sorted column, S = ceil(n / D3P_CS_STAGE), is staged in LDS (32 KiB at most); lo = #{keys < k} and
// hi = #{keys <= k} come from a binary search there and one in a window of S - 1 keys of the sorted column in memory (cs_count);
// ranks2 = lo + hi + 1, 0 in a column that holds a NaN (read off the column's ends), written column-major to W1 and brought to the
// row-major output by k_cs_rank_rows, the mirror of k_cs_keys.
//
// THE DISTANCES (k_cdf_part, k_cdf_merge).  With i = #{a <= v}, j = #{b <= v} over the pooled values v, per column
//   ks_num = max_v |i n_b - j n_a|        ks_at = the smallest v that attains it        w1 = sum_v |i / n_a - j / n_b| (next(v) - v)
// A thread at position p of a acts if p is the last of its run of equal keys: i = p + 1, j by cs_count in b, next = the smaller of
// a[p + 1] and b[j].  The blocks of b follow: a position acts if it is the last of its run and its key does not occur in a.  Every pooled
// value is visited once.  ORDER OF w1: term = ((double)num / ((double)n_a (double)n_b)) ((double)next - (double)v); a thread adds the
// terms of its positions blk T + r 256 + t in ascending r onto +0; the 256 threads merge in the tree red[t] += red[t + w], w = 128, 64,
// .. 1; k_cdf_merge adds the blocks' partials in ascending order, a's then b's, onto +0: one thread per column.  No atomics; the bits
// are a function of the two columns alone.  ERROR: a term carries five roundings (num, the denominator, the quotient, the difference,
// the product), a thread's chain at most 16, the tree 8, the merge nblk_a + nblk_b: |w1 - exact| <= gamma_k sum |term| with k =
// d3p_column_cdf_distance_roundings(n_a, n_b) = 29 + nblk_a + nblk_b and gamma_k = k u / (1 - k u), u = 2^-53.
// FLAGS are read off the ends of the sorted columns: a NaN (float32: the first word a negative NaN or the last a positive one) in either
// table gives ks_num = 2^64 - 1, ks_at = NaN, w1 = NaN; an infinity without a NaN leaves ks_num and ks_at as computed and gives w1 = NaN.
//
// Static LDS only, integer LDS operations only (the float64 tree of k_cdf_part is plain loads and stores); no scratch.
#pragma once
#include "d3p_sort_columns.h"

namespace d3p {

__device__ inline uint32_t cs_stored(uint32_t k, int32_t dtype) { return dtype ? (uint32_t)i32_of_key(k) : __float_as_uint(f32_of_key(k)); }
__device__ inline double cs_value(uint32_t k, int32_t dtype) { return dtype ? (double)i32_of_key(k) : (double)f32_of_key(k); }

// exclusive scan of v over the 256 threads of a workgroup (s4: 4 words of LDS; two barriers)
__device__ inline uint32_t cs_block_excl(uint32_t v, uint32_t* s4, int t)
{
    const int lane = t & 63, w = t >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) s4[w] = incl;
    __syncthreads();
    uint32_t off = 0u;
    for (int i = 0; i < w; ++i) off += s4[i];
    __syncthreads();
    return off + incl - v;
}

// #{i < n : key(sc[i]) < k} (LE false) or <= k (LE true) of a sorted column sc whose every S-th key is staged in st[0 .. m), m = ceil(n / S)
template <bool LE>
__device__ inline uint32_t cs_count(const uint32_t* st, uint32_t m, uint32_t S, const uint32_t* sc, uint32_t n, int32_t dtype, uint32_t k)
{
    uint32_t lo = 0u, hi = m;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1, x = st[mid];
        if (LE ? x <= k : x < k) lo = mid + 1u; else hi = mid;
    }
    if (lo == 0u || S == 1u) return lo;
    // sc[(lo - 1) S] is below, sc[lo S] (if there) is not: the answer lies in ((lo - 1) S, min(lo S, n)]
    const uint64_t end = (uint64_t)lo * S;
    uint32_t l = (lo - 1u) * S + 1u, h = end < n ? (uint32_t)end : n;
    while (l < h) {
        const uint32_t mid = l + ((h - l) >> 1), x = key_of(sc[mid], dtype);
        if (LE ? x <= k : x < k) l = mid + 1u; else h = mid;
    }
    return l;
}

// ---- launch 0: the keys, column-major -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cs_keys(CsArgs a)
{
    __shared__ uint32_t tile[64][65];
    const uint32_t tiles_c = (a.d + 63u) / 64u;
    const uint32_t r0 = (blockIdx.x / tiles_c) * 64u, c0 = (blockIdx.x % tiles_c) * 64u;
    const uint32_t l = threadIdx.x & 63u, q = threadIdx.x >> 6;
#pragma unroll 4
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t r = r0 + q + 4u * i, c = c0 + l;
        tile[q + 4u * i][l] = (r < a.n && c < a.d) ? key_of(a.x[(size_t)r * (size_t)a.ld + c], a.dtype) : 0u;
    }
    __syncthreads();
#pragma unroll 4
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t c = c0 + q + 4u * i, r = r0 + l;
        if (r < a.n && c < a.d) a.w0[(size_t)c * a.n + r] = tile[l][q + 4u * i];
    }
}

// the mirror: the column-major doubled midranks of W1 to the row-major output
__global__ __launch_bounds__(256) void k_cs_rank_rows(CsArgs a)
{
    __shared__ uint32_t tile[64][65];
    const uint32_t tiles_c = (a.d + 63u) / 64u;
    const uint32_t r0 = (blockIdx.x / tiles_c) * 64u, c0 = (blockIdx.x % tiles_c) * 64u;
    const uint32_t l = threadIdx.x & 63u, q = threadIdx.x >> 6;
#pragma unroll 4
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t c = c0 + q + 4u * i, r = r0 + l;
        tile[q + 4u * i][l] = (r < a.n && c < a.d) ? a.w1[(size_t)c * a.n + r] : 0u;
    }
    __syncthreads();
#pragma unroll 4
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t r = r0 + q + 4u * i, c = c0 + l;
        if (r < a.n && c < a.d) a.ranks2[(size_t)r * (size_t)a.ld_r + c] = (int32_t)tile[l][q + 4u * i];
    }
}

// ---- one pass: counts, scan, scatter ----------------------------------------------------------------------------------------------------
struct CsPass {
    const uint32_t* src;   // d x ld_src keys
    uint32_t* dst;         // d x ld_dst
    int64_t ld_src, ld_dst;
    uint32_t* hist;
    uint32_t n, nblk;
    int32_t shift, last, dtype;
};

__global__ __launch_bounds__(256) void k_cs_hist(CsPass p)
{
    __shared__ uint32_t h[4][256];
    const uint32_t c = blockIdx.x / p.nblk, b = blockIdx.x % p.nblk;
    const uint32_t t = threadIdx.x, w = t >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i][t] = 0u;
    __syncthreads();
    const uint32_t* col = p.src + (size_t)c * (size_t)p.ld_src;
    const uint32_t base = b * D3P_CS_T;
#pragma unroll 4
    for (uint32_t i = 0; i < D3P_CS_THREAD_KEYS; ++i) {
        const uint32_t idx = base + i * 256u + t;
        if (idx < p.n) atomicAdd(&h[w][(col[idx] >> p.shift) & 255u], 1u);
    }
    __syncthreads();
    p.hist[((size_t)c * 256u + t) * p.nblk + b] = h[0][t] + h[1][t] + h[2][t] + h[3][t];
}

__global__ __launch_bounds__(256) void k_cs_scan(CsPass p)
{
    __shared__ uint32_t s4[4];
    const uint32_t t = threadIdx.x;
    uint32_t* h = p.hist + ((size_t)blockIdx.x * 256u + t) * p.nblk;
    uint32_t sum = 0u;
    for (uint32_t b = 0; b < p.nblk; ++b) sum += h[b];
    uint32_t run = cs_block_excl(sum, s4, (int)t);
    for (uint32_t b = 0; b < p.nblk; ++b) {
        const uint32_t v = h[b];
        h[b] = run;
        run += v;
    }
}

__global__ __launch_bounds__(256) void k_cs_scatter(CsPass p)
{
    __shared__ uint32_t keys[D3P_CS_T];
    __shared__ uint32_t wcnt[4][256];
    __shared__ uint32_t dstart[256], gbase[256], s4[4];
    const uint32_t c = blockIdx.x / p.nblk, b = blockIdx.x % p.nblk;
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) wcnt[i][t] = 0u;
    __syncthreads();
    const uint32_t* col = p.src + (size_t)c * (size_t)p.ld_src;
    const uint32_t first = b * D3P_CS_T + w * 1024u + lane;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t k[D3P_CS_THREAD_KEYS], pos[D3P_CS_THREAD_KEYS];
#pragma unroll
    for (uint32_t r = 0; r < D3P_CS_THREAD_KEYS; ++r) {
        const uint32_t idx = first + r * 64u;
        const bool valid = idx < p.n;
        k[r] = valid ? col[idx] : 0xffffffffu;
        const uint32_t dg = (k[r] >> p.shift) & 255u;
        uint64_t m = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (dg >> bit) & 1u;
            const uint64_t bal = __ballot(one);
            m &= one ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(m & below);
        const uint32_t run = wcnt[w][dg];
        pos[r] = run + rank;
        __builtin_amdgcn_wave_barrier();   // (every lane has read the running count before the round's first lane of a digit moves it)
        if (valid && rank == 0u) wcnt[w][dg] = run + (uint32_t)__popcll(m);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // thread t = digit t: the block's digit starts and each wavefront's offset inside the digit's run
    const uint32_t c0 = wcnt[0][t], c1 = wcnt[1][t], c2 = wcnt[2][t], c3 = wcnt[3][t];
    const uint32_t start = cs_block_excl(c0 + c1 + c2 + c3, s4, (int)t);
    dstart[t] = start;
    gbase[t] = p.hist[((size_t)c * 256u + t) * p.nblk + b];
    wcnt[0][t] = start; wcnt[1][t] = start + c0; wcnt[2][t] = start + c0 + c1; wcnt[3][t] = start + c0 + c1 + c2;
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < D3P_CS_THREAD_KEYS; ++r)
        if (first + r * 64u < p.n) keys[wcnt[w][(k[r] >> p.shift) & 255u] + pos[r]] = k[r];
    __syncthreads();
    const uint32_t left = p.n - b * D3P_CS_T, cnt = left < D3P_CS_T ? left : D3P_CS_T;
    uint32_t* out = p.dst + (size_t)c * (size_t)p.ld_dst;
    for (uint32_t i = t; i < cnt; i += 256u) {
        const uint32_t key = keys[i], dg = (key >> p.shift) & 255u;
        out[gbase[dg] + (i - dstart[dg])] = p.last ? cs_stored(key, p.dtype) : key;
    }
}

// ---- the doubled midranks -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cs_ranks(CsArgs a, uint32_t S, uint32_t nstrips)
{
    __shared__ uint32_t st[D3P_CS_STAGE];
    const uint32_t c = blockIdx.x / nstrips, strip = blockIdx.x % nstrips, t = threadIdx.x;
    const uint32_t n = a.n, m = (n + S - 1u) / S;
    const uint32_t* sc = a.out + (size_t)c * (size_t)a.ld_s;
    for (uint32_t j = t; j < m; j += 256u) st[j] = key_of(sc[(size_t)j * S], a.dtype);
    const bool nan = !a.dtype && (word_is_nan(sc[0]) || word_is_nan(sc[n - 1u]));
    __syncthreads();
    const uint32_t* kc = a.w0 + (size_t)c * n;
    uint32_t* rc = a.w1 + (size_t)c * n;
    const uint32_t p0 = strip * D3P_CS_RANK_STRIP, left = n - p0, cnt = left < D3P_CS_RANK_STRIP ? left : D3P_CS_RANK_STRIP;
    for (uint32_t i = t; i < cnt; i += 256u) {
        const uint32_t k = kc[p0 + i];
        const uint32_t lo = cs_count<false>(st, m, S, sc, n, a.dtype, k), hi = cs_count<true>(st, m, S, sc, n, a.dtype, k);
        rc[p0 + i] = nan ? 0u : lo + hi + 1u;
    }
}

// ---- KS and Wasserstein-1 of two sorted tables ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cdf_part(CdfArgs g, uint32_t S_a, uint32_t S_b)
{
#pragma clang fp contract(off)
    __shared__ uint32_t st[D3P_CS_STAGE];
    __shared__ double red[256];
    __shared__ uint64_t rnum[256];
    __shared__ uint32_t rkey[256];
    const uint32_t nbt = g.nblk_a + g.nblk_b;
    const uint32_t c = blockIdx.x / nbt, bb = blockIdx.x % nbt, t = threadIdx.x;
    const bool side = bb >= g.nblk_a;                                  // false: a block of a; true: a block of b
    const uint32_t blk = side ? bb - g.nblk_a : bb;
    const uint32_t* ca = g.a + (size_t)c * (size_t)g.ld_a;
    const uint32_t* cb = g.b + (size_t)c * (size_t)g.ld_b;
    const uint32_t* self = side ? cb : ca;
    const uint32_t* other = side ? ca : cb;
    const uint32_t n_s = side ? g.n_b : g.n_a, n_o = side ? g.n_a : g.n_b, S = side ? S_a : S_b;
    const uint32_t m = (n_o + S - 1u) / S;
    const int32_t dtype = g.dtype;
    for (uint32_t j = t; j < m; j += 256u) st[j] = key_of(other[(size_t)j * S], dtype);
    __syncthreads();
    const double denom = (double)g.n_a * (double)g.n_b;
    double acc = 0.0;
    uint64_t best = 0ull;
    uint32_t best_key = 0xffffffffu;
    for (uint32_t r = 0; r < D3P_CS_THREAD_KEYS; ++r) {
        const uint32_t p = blk * D3P_CS_T + r * 256u + t;
        if (p >= n_s) break;
        const uint32_t kv = key_of(self[p], dtype);
        const bool more = p + 1u < n_s;
        const uint32_t kn_self = more ? key_of(self[p + 1u], dtype) : 0u;
        if (more && kn_self == kv) continue;                           // not the last of its run
        const uint32_t cnt = cs_count<true>(st, m, S, other, n_o, dtype, kv);
        if (side && cnt > 0u && key_of(other[cnt - 1u], dtype) == kv) continue;   // the value occurs in a: a's thread has it
        const uint64_t i = side ? cnt : p + 1u, j = side ? p + 1u : cnt;
        const uint64_t x = i * g.n_b, y = j * g.n_a, num = x > y ? x - y : y - x;
        if (num > best || (num == best && kv < best_key)) { best = num; best_key = kv; }
        bool has = more;
        uint32_t kn = kn_self;
        if (cnt < n_o) {
            const uint32_t ko = key_of(other[cnt], dtype);
            if (!has || ko < kn) kn = ko;
            has = true;
        }
        if (has) {
            const double term = ((double)num / denom) * (cs_value(kn, dtype) - cs_value(kv, dtype));
            acc = acc + term;
        }
    }
    red[t] = acc; rnum[t] = best; rkey[t] = best_key;
    __syncthreads();
    for (uint32_t w = 128u; w > 0u; w >>= 1) {
        if (t < w) {
            red[t] = red[t] + red[t + w];
            const uint64_t on = rnum[t + w];
            const uint32_t ok = rkey[t + w];
            if (on > rnum[t] || (on == rnum[t] && ok < rkey[t])) { rnum[t] = on; rkey[t] = ok; }
        }
        __syncthreads();
    }
    if (t == 0u) {
        const size_t at = (size_t)c * nbt + bb;
        g.part_w1[at] = red[0]; g.part_num[at] = rnum[0]; g.part_key[at] = rkey[0];
    }
}

__global__ __launch_bounds__(64) void k_cdf_merge(CdfArgs g)
{
#pragma clang fp contract(off)
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= g.d) return;
    const uint32_t nbt = g.nblk_a + g.nblk_b;
    const uint32_t* ca = g.a + (size_t)c * (size_t)g.ld_a;
    const uint32_t* cb = g.b + (size_t)c * (size_t)g.ld_b;
    const uint32_t e0 = ca[0], e1 = ca[g.n_a - 1u], e2 = cb[0], e3 = cb[g.n_b - 1u];
    const bool nan = !g.dtype && (word_is_nan(e0) || word_is_nan(e1) || word_is_nan(e2) || word_is_nan(e3));
    const bool inf = !g.dtype && !(word_is_finite(e0) && word_is_finite(e1) && word_is_finite(e2) && word_is_finite(e3));
    double w = 0.0;
    uint64_t best = 0ull;
    uint32_t best_key = 0xffffffffu;
    for (uint32_t b = 0; b < nbt; ++b) {
        const size_t at = (size_t)c * nbt + b;
        w = w + g.part_w1[at];
        const uint64_t on = g.part_num[at];
        const uint32_t ok = g.part_key[at];
        if (on > best || (on == best && ok < best_key)) { best = on; best_key = ok; }
    }
    g.ks_num[c] = nan ? ~0ull : best;
    g.ks_at[c] = nan ? 0x7fc00000u : cs_stored(best_key, g.dtype);
    g.w1[c] = (nan || inf) ? (double)NAN : w;
}

// ---- the launches -------------------------------------------------------------------------------------------------------------------------
int cs_sort_launch(const char* what, hipStream_t s, const CsArgs& a)
{
    const unsigned tiles = (unsigned)(((uint64_t)(a.n + 63u) / 64u) * ((a.d + 63u) / 64u)), blocks = a.d * a.nblk;
    hipLaunchKernelGGL(k_cs_keys, dim3(tiles), dim3(256), 0, s, a);
    int rc = check_launch(what);
    if (rc != D3P_OK) return rc;
    CsPass p;
    p.hist = a.hist; p.n = a.n; p.nblk = a.nblk; p.dtype = a.dtype;
    for (int pass = 0; pass < 4; ++pass) {
        p.src = pass == 0 ? a.w0 : (pass == 2 ? a.out : a.w1);
        p.dst = (pass & 1) ? a.out : a.w1;
        p.ld_src = pass == 2 ? a.ld_s : (int64_t)a.n;
        p.ld_dst = (pass & 1) ? a.ld_s : (int64_t)a.n;
        p.shift = 8 * pass; p.last = pass == 3;
        hipLaunchKernelGGL(k_cs_hist, dim3(blocks), dim3(256), 0, s, p);
        if ((rc = check_launch(what)) != D3P_OK) return rc;
        hipLaunchKernelGGL(k_cs_scan, dim3(a.d), dim3(256), 0, s, p);
        if ((rc = check_launch(what)) != D3P_OK) return rc;
        hipLaunchKernelGGL(k_cs_scatter, dim3(blocks), dim3(256), 0, s, p);
        if ((rc = check_launch(what)) != D3P_OK) return rc;
    }
    if (!a.ranks2) return D3P_OK;
    const uint32_t nstrips = (uint32_t)(((uint64_t)a.n + D3P_CS_RANK_STRIP - 1u) / D3P_CS_RANK_STRIP);
    hipLaunchKernelGGL(k_cs_ranks, dim3(a.d * nstrips), dim3(256), 0, s, a, cs_stride(a.n), nstrips);
    if ((rc = check_launch(what)) != D3P_OK) return rc;
    hipLaunchKernelGGL(k_cs_rank_rows, dim3(tiles), dim3(256), 0, s, a);
    return check_launch(what);
}

int cs_cdf_launch(const char* what, hipStream_t s, const CdfArgs& g)
{
    hipLaunchKernelGGL(k_cdf_part, dim3(g.d * (g.nblk_a + g.nblk_b)), dim3(256), 0, s, g, cs_stride(g.n_a), cs_stride(g.n_b));
    const int rc = check_launch(what);
    if (rc != D3P_OK) return rc;
    hipLaunchKernelGGL(k_cdf_merge, dim3((g.d + 63u) / 64u), dim3(64), 0, s, g);
    return check_launch(what);
}

}  // namespace d3p
