// Classification metrics of a fitted logistic regression (d3p_amd/classification.py).  Two entries, both of
// which compute INTEGERS only -- counts, pair counts, fixed-point sums -- so that no summation order has to be promised: any grid and
// any order of the integer atomic adds below gives the same bits, and every result is compared by value.
//
// d3p_predict_confusion: per posterior draw s, counts over the ROWS r of a table.  t = the product tile's value (+ the intercept), as for
// every user of the tile:
//   mu = the float32 mean d3p_predict_mean_rows stores: glm_mean<D3P_FAMILY_LOGREG> (d3p_glm_tile.h)
//   v  = the 0 / 1 label d3p_predict_logreg stores: glm_outcome<D3P_FAMILY_LOGREG> (d3p_outcome.h) on the same obs keys, rows and r
//   out[0 n + s] = #{r : (float)v == y_r}      out[1 n + s] = #{r : mu is NaN}
//   out[(2 + 2 j) n + s] = #{r : mu >= tau_j and y_r == 1}      out[(3 + 2 j) n + s] = #{r : mu >= tau_j and y_r == 0}      (j < T <= 4)
// k_predict_confusion has k_predict_discrepancy's shape (d3p_discrepancy.hip): grid (row strips, tiles of 128 draws), tile_product per
// row tile, tile_scatter per draw half under `unroll 1`, lane = draw l % 32 and row half l / 32 walking 32 rows on 32 distinct LDS
// banks, the draws' obs keys in LDS once per workgroup, the tile's 128 labels in LDS once per row tile.  Each lane keeps uint32 counts in
// registers across its strip; the four row quarters of a draw meet in LDS (the tile's smem again) and one thread per draw adds the
// strip's total onto out with 64-bit integer atomic adds; the entry zeroes out on the stream first.  No workspace, no second launch.
//
// d3p_binary_curve: the ROC histogram and the reliability table of ONE score vector p (float32 in [0, 1]) against labels y (int32 in
// {0, 1}), model-free.  The bin of a score comes from its bit pattern (non-negative float32 patterns are ordered as the values are):
//   c(x) = float_as_uint(x) >> 12      bin(p) = c(p) for p < 0.5f, 2 * 0x3F000 - c(1.0f - p) otherwise      (1.0f - p is exact there)
// which keeps 11 mantissa bits of min(p, 1 - p) at BOTH ends.  k_curve_hist adds into hist[2][D3P_CURVE_BINS] (equal bins of a
// wavefront are added once) and into calib[3][B]; k_curve_chunks and k_curve_totals turn hist into P, N, the two pair counts and the
// numerator of the Kolmogorov-Smirnov statistic.
#include "d3p_device.h"
#include "d3p_glm_tile.h"
#include "d3p_host.h"
#include "d3p_outcome.h"

namespace d3p {

// (D3P_CONF_THRESHOLDS = 4, D3P_CONF_COUNTS = 10, D3P_CURVE_BINS = 0x7E001 and D3P_CURVE_SUMMARY = 6: include/d3p_hip.h)
#define D3P_CONF_DEFAULT_STRIPS 512  // the siblings' cap; ANY value gives the same counts (integers): d3p_predict_confusion_set_strips

static uint32_t g_conf_max_strips = D3P_CONF_DEFAULT_STRIPS;

struct ConfusionArgs {
    const float* X;
    const float* y;
    uint64_t rows;
    int d, w_off, b_col;
    const float* lat;
    int64_t ld;
    uint32_t n;
    const uint32_t* obs_keys;
    float tau[D3P_CONF_THRESHOLDS];   // slots >= T hold NaN: they count nothing
    uint32_t tiles, per;
    unsigned long long* out;          // [D3P_CONF_COUNTS][n], zeroed on the stream before the launch
};

// one (draw, strip, quarter) set of counts.  uint32 cannot overflow: a lane sees each row of its strip at most once per draw and a row
// adds at most 1 to a count, so every count is <= the strip's rows <= rows < 2^32.
struct ConfAcc {
    uint32_t agree, nan, tp[D3P_CONF_THRESHOLDS], fp[D3P_CONF_THRESHOLDS];
};

__device__ __forceinline__ void conf_init(ConfAcc& a)
{
    a.agree = 0u; a.nan = 0u;
#pragma unroll
    for (int j = 0; j < D3P_CONF_THRESHOLDS; ++j) { a.tp[j] = 0u; a.fp[j] = 0u; }
}

// red: [count][quarter][draw of the tile] uint32, 10 x 4 x 128
__device__ __forceinline__ void conf_put(uint32_t* red, int q, int dl, const ConfAcc& a)
{
    red[(0 * 4 + q) * D3P_TILE_M + dl] = a.agree;
    red[(1 * 4 + q) * D3P_TILE_M + dl] = a.nan;
#pragma unroll
    for (int j = 0; j < D3P_CONF_THRESHOLDS; ++j) {
        red[((2 + 2 * j) * 4 + q) * D3P_TILE_M + dl] = a.tp[j];
        red[((3 + 2 * j) * 4 + q) * D3P_TILE_M + dl] = a.fp[j];
    }
}

// Registers: one wave per SIMD as its sibling; the figures: docs/experiments_classification.md
__global__ void __launch_bounds__(256, 1) k_predict_confusion(ConfusionArgs g)
{
    // [k][draw] | [k][row] during the product; then each wave's t, half a tile at a time (4 x 32 x 65 floats); at the end 10 x 4 x 128 uint32
    __shared__ __attribute__((aligned(16))) float smem[D3P_TILE_SMEM];
    static_assert(sizeof(float) * D3P_TILE_SMEM >= sizeof(uint32_t) * D3P_CONF_COUNTS * 4 * D3P_TILE_M, "the quarter merge fits");
    __shared__ uint32_t keys[D3P_TILE_M][4];   // per draw of the tile: the obs key
    __shared__ float ys[D3P_TILE_N];           // the row tile's labels
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int i = lane & 31, h = lane >> 5;            // the lane's draw within a half of the wave's draws; its half of the wave's rows
    const int col = wn * 64 + h * 32;                  // first of the lane's 32 rows within a tile: quarter q = 2 wn + h
    const uint32_t s0 = blockIdx.y * D3P_TILE_M;
    const uint32_t t_lo = blockIdx.x * g.per;          // the tiles [t_lo, t_hi) of the workgroup's strip (grid x = strips)
    const uint32_t t_hi = t_lo + g.per < g.tiles ? t_lo + g.per : g.tiles;
    stage_obs_keys<D3P_FAMILY_LOGREG>(keys, g.obs_keys, s0, g.n);
    const float tau0 = g.tau[0], tau1 = g.tau[1], tau2 = g.tau[2], tau3 = g.tau[3];
    ConfAcc a0, a1;
    conf_init(a0);
    conf_init(a1);
    for (uint32_t t = t_lo; t < t_hi; ++t) {
        const uint64_t r0 = (uint64_t)t * D3P_TILE_N;
        if (tid < D3P_TILE_N) {   // (the product's barriers come between this and its readers; the last readers are behind a barrier)
            const uint64_t r = r0 + tid;
            ys[tid] = r < g.rows ? g.y[r] : -1.f;
        }
        tile_f16v acc[2][2];
        tile_product(smem, g, r0, s0, acc);
        float* L = tile_block(smem);
        const uint64_t ahead = g.rows - r0;   // >= 1; the live rows among the lane's 32 rows r0 + col .. r0 + col + 31:
        const int jn = ahead <= (uint64_t)col ? 0 : (ahead - col >= 32 ? 32 : (int)(ahead - col));
#pragma unroll 1
        for (int mb = 0; mb < 2; ++mb) {
            tile_scatter(L, mb == 0 ? acc[0][0] : acc[1][0], mb == 0 ? acc[0][1] : acc[1][1]);   // (selected by hand: the loop is not unrolled)
            __syncthreads();
            const int sl = wm * 64 + mb * 32 + i;
            const uint32_t s = s0 + sl;
            if (s < g.n) {
                ConfAcc a = mb == 0 ? a0 : a1;
                const float b = g.b_col >= 0 ? g.lat[(size_t)s * g.ld + g.b_col] : 0.f;
                const uint32_t o0 = keys[sl][0], o1 = keys[sl][1];
                const float* p = L + i * 65 + h * 32;
                const uint64_t rb = r0 + col;
#pragma unroll 1
                for (int j = 0; j < jn; ++j) {
                    float tv = p[j];
                    if (g.b_col >= 0) tv = tv + b;
                    const float mu = glm_mean<D3P_FAMILY_LOGREG>(tv);
                    const float yr = ys[col + j];
                    const uint32_t pos = yr == 1.0f ? 1u : 0u, neg = yr == 0.0f ? 1u : 0u;
                    const int32_t v = glm_outcome<D3P_FAMILY_LOGREG>(tv, o0, o1, 0u, 0u, g.rows, rb + j, 0.f);
                    a.agree += (float)v == yr ? 1u : 0u;
                    a.nan += mu != mu ? 1u : 0u;
                    const uint32_t g0 = mu >= tau0 ? 1u : 0u, g1 = mu >= tau1 ? 1u : 0u, g2 = mu >= tau2 ? 1u : 0u, g3 = mu >= tau3 ? 1u : 0u;
                    a.tp[0] += g0 & pos; a.fp[0] += g0 & neg;
                    a.tp[1] += g1 & pos; a.fp[1] += g1 & neg;
                    a.tp[2] += g2 & pos; a.fp[2] += g2 & neg;
                    a.tp[3] += g3 & pos; a.fp[3] += g3 & neg;
                }
                if (mb == 0) a0 = a; else a1 = a;
            }
            __syncthreads();
        }
    }
    uint32_t* red = reinterpret_cast<uint32_t*>(smem);   // [count][q][draw of the tile]
    conf_put(red, wn * 2 + h, wm * 64 + i, a0);
    conf_put(red, wn * 2 + h, wm * 64 + 32 + i, a1);
    __syncthreads();
    if (tid < D3P_TILE_M && s0 + tid < g.n) {   // the four quarters of draw tid, widened, onto out[count][n]: integer adds, any order
        unsigned long long* o = g.out + s0 + tid;
#pragma unroll
        for (int k = 0; k < D3P_CONF_COUNTS; ++k) {
            const uint32_t* r = red + k * 4 * D3P_TILE_M + tid;
            const unsigned long long c = (unsigned long long)r[0] + r[D3P_TILE_M] + r[2 * D3P_TILE_M] + r[3 * D3P_TILE_M];
            if (c) atomicAdd(o + k * (size_t)g.n, c);
        }
    }
}

// ---- the curve of one score vector ----------------------------------------------------------------------------------------------------
#define D3P_CURVE_MAX_CALIB 64
#define D3P_CURVE_CHUNK 2048                                                        // bins per workgroup of k_curve_chunks: 256 threads x 8
#define D3P_CURVE_CHUNKS ((D3P_CURVE_BINS + D3P_CURVE_CHUNK - 1) / D3P_CURVE_CHUNK)   // 253
static_assert(D3P_CURVE_CHUNKS <= 256, "k_curve_totals takes one chunk per thread");

// the strictly order-preserving map of the file comment; p in [0, 1], -0.0f as 0
__device__ __forceinline__ uint32_t curve_bin(float p)
{
    p = p + 0.0f;   // -0.0f -> +0.0f
    return p < 0.5f ? (__float_as_uint(p) >> 12) : 2u * 0x3F000u - (__float_as_uint(1.0f - p) >> 12);
}

// hist[class][bin] += 1 and calib[0 | 1 | 2][b] += 1 | y | (uint64)((double)p 2^36) per valid row; summary[0] += the invalid rows.
// Equal (class, bin) keys of a wavefront are peeled off one key at a time and added once with their count, so a vector of one
// repeated score costs one global add per wavefront, not 64 on one address.  calib meets in LDS and is flushed once per workgroup.
__global__ void __launch_bounds__(256) k_curve_hist(const float* p, const int32_t* y, uint64_t rows, uint32_t B, uint32_t* hist,
                                                    unsigned long long* calib, unsigned long long* summary)
{
    __shared__ uint32_t cnt[2][D3P_CURVE_MAX_CALIB];            // per reliability bin: rows, positives (a workgroup sees < 2^32 rows)
    __shared__ unsigned long long fix[D3P_CURVE_MAX_CALIB];     // ... and the fixed-point sum of the scores
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < D3P_CURVE_MAX_CALIB) { cnt[0][tid] = 0u; cnt[1][tid] = 0u; fix[tid] = 0ull; }
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    const uint64_t span = (rows + 255u) / 256u * 256u;   // whole wavefronts walk the loop together: the ballots below see all 64 lanes
    uint32_t bad = 0u;
    for (uint64_t r = (uint64_t)blockIdx.x * 256u + tid; r < span; r += step) {
        const bool live = r < rows;
        const float x = live ? p[r] : 0.f;
        const int32_t c = live ? y[r] : 0;
        const bool ok = live && x >= 0.0f && x <= 1.0f && (c == 0 || c == 1);   // (a NaN fails both comparisons)
        bad += live && !ok ? 1u : 0u;
        uint32_t key = 0xFFFFFFFFu;
        if (ok) {
            key = (uint32_t)c * D3P_CURVE_BINS + curve_bin(x);
            const float xb = (x + 0.0f) * (float)B;
            const uint32_t b = (uint32_t)(int)xb < B - 1u ? (uint32_t)(int)xb : B - 1u;
            atomicAdd(&cnt[0][b], 1u);
            if (c) atomicAdd(&cnt[1][b], 1u);
            atomicAdd(&fix[b], (unsigned long long)((double)x * 68719476736.0));
        }
        unsigned long long active = __ballot(ok);
        while (active) {   // (uniform: `active` is the same in every lane)
            const int leader = __ffsll(active) - 1;
            const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
            const unsigned long long m = __ballot(ok && key == k);
            if (lane == leader) atomicAdd(hist + k, (uint32_t)__popcll(m));
            active &= ~m;
        }
    }
    if (bad) atomicAdd(summary, (unsigned long long)bad);   // (rare: the Python layer refuses such a vector)
    __syncthreads();
    if ((uint32_t)tid < B && cnt[0][tid]) {
        atomicAdd(calib + tid, (unsigned long long)cnt[0][tid]);
        if (cnt[1][tid]) atomicAdd(calib + B + tid, (unsigned long long)cnt[1][tid]);
        if (fix[tid]) atomicAdd(calib + 2 * (size_t)B + tid, fix[tid]);
    }
}

// inclusive sum over the workgroup's 256 threads of x (uint32: every prefix is <= rows <= 2^27); scratch: 4 words
__device__ __forceinline__ uint32_t block_scan_256(uint32_t x, uint32_t* scratch, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t v = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, off);
        if (lane >= off) v += u;
    }
    if (lane == 63) scratch[wave] = v;
    __syncthreads();
    uint32_t before = 0u;
    total = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t s = scratch[w];
        if (w < wave) before += s;
        total += s;
    }
    __syncthreads();
    return v + before;
}

// Chunk c = the bins [2048 c, 2048 c + 2048): chunk_tot[2 c] = its positives, chunk_tot[2 c + 1] = its negatives; onto summary[3] the
// pairs ordered WITHIN the chunk, sum_b pos_b #{negatives of the chunk's bins below b}, onto summary[4] sum_b pos_b neg_b.
__global__ void __launch_bounds__(256) k_curve_chunks(const uint32_t* hist, unsigned long long* chunk_tot, unsigned long long* summary)
{
    __shared__ uint32_t scratch[4];
    __shared__ unsigned long long pairs[2];
    const int tid = threadIdx.x;
    if (tid < 2) pairs[tid] = 0ull;
    const uint32_t base = blockIdx.x * D3P_CURVE_CHUNK + tid * 8u;
    uint32_t neg[8], pos[8], nsum = 0u, psum = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t b = base + j;
        neg[j] = b < D3P_CURVE_BINS ? hist[b] : 0u;
        pos[j] = b < D3P_CURVE_BINS ? hist[D3P_CURVE_BINS + b] : 0u;
        nsum += neg[j];
        psum += pos[j];
    }
    uint32_t ntot, ptot;
    uint32_t below = block_scan_256(nsum, scratch, ntot) - nsum;   // the chunk's negatives in the bins below this thread's
    (void)block_scan_256(psum, scratch, ptot);
    unsigned long long conc = 0ull, same = 0ull;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        conc += (unsigned long long)pos[j] * below;
        same += (unsigned long long)pos[j] * neg[j];
        below += neg[j];
    }
    if (conc) atomicAdd(&pairs[0], conc);
    if (same) atomicAdd(&pairs[1], same);
    __syncthreads();
    if (tid == 0) {
        chunk_tot[2 * blockIdx.x] = ptot;
        chunk_tot[2 * blockIdx.x + 1] = ntot;
        if (pairs[0]) atomicAdd(summary + 3, pairs[0]);
        if (pairs[1]) atomicAdd(summary + 4, pairs[1]);
    }
}

// One workgroup per chunk again, now that every chunk's totals are known.  Each scans the 253 chunk totals (cheap) for P, N and the
// positives / negatives of the chunks below its own, then walks its 2048 bins ascending: with a_k / b_k the positives / negatives of the
// bins 0..k, onto summary[5] the maximum of |b_k P - a_k N| -- the numerator of the Kolmogorov-Smirnov statistic max |tpr - fpr| over
// the bin edges (counted from the bottom; from the top it is the same set of values).  Workgroup 0 also writes summary[1] = P,
// summary[2] = N and adds onto summary[3] the pairs ordered ACROSS chunks, sum_c P_c #{negatives of the chunks below c}.
__global__ void __launch_bounds__(256) k_curve_totals(const uint32_t* hist, const unsigned long long* chunk_tot, unsigned long long* summary)
{
    __shared__ uint32_t scratch[4];
    __shared__ unsigned long long cross, top;
    __shared__ uint32_t mine[2];
    const int tid = threadIdx.x;
    if (tid == 0) { cross = 0ull; top = 0ull; }
    const uint32_t pc = tid < D3P_CURVE_CHUNKS ? (uint32_t)chunk_tot[2 * tid] : 0u;
    const uint32_t nc = tid < D3P_CURVE_CHUNKS ? (uint32_t)chunk_tot[2 * tid + 1] : 0u;
    uint32_t N, P;
    const uint32_t nbelow = block_scan_256(nc, scratch, N) - nc;
    const uint32_t pbelow = block_scan_256(pc, scratch, P) - pc;
    if ((uint32_t)tid == blockIdx.x) { mine[0] = pbelow; mine[1] = nbelow; }
    if (blockIdx.x == 0) {
        const unsigned long long x = (unsigned long long)pc * nbelow;
        if (x) atomicAdd(&cross, x);
    }
    const uint32_t base = blockIdx.x * D3P_CURVE_CHUNK + tid * 8u;
    uint32_t neg[8], pos[8], nsum = 0u, psum = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t b = base + j;
        neg[j] = b < D3P_CURVE_BINS ? hist[b] : 0u;
        pos[j] = b < D3P_CURVE_BINS ? hist[D3P_CURVE_BINS + b] : 0u;
        nsum += neg[j];
        psum += pos[j];
    }
    uint32_t t0, t1;
    uint32_t bk = block_scan_256(nsum, scratch, t0) - nsum;   // (the scans' barriers also publish `mine`)
    uint32_t ak = block_scan_256(psum, scratch, t1) - psum;
    ak += mine[0];
    bk += mine[1];
    unsigned long long best = 0ull;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        ak += pos[j];
        bk += neg[j];
        const unsigned long long u = (unsigned long long)bk * P, v = (unsigned long long)ak * N;   // both < 2^54
        const unsigned long long gap = u > v ? u - v : v - u;
        best = gap > best ? gap : best;
    }
    if (best) atomicMax(&top, best);
    __syncthreads();
    if (tid == 0) {
        if (top) atomicMax(summary + 5, top);
        if (blockIdx.x == 0) {
            summary[1] = P;
            summary[2] = N;
            if (cross) atomicAdd(summary + 3, cross);   // (k_curve_chunks' adds are complete: the launches are ordered on the stream)
        }
    }
}

}  // namespace d3p

using namespace d3p;

extern "C" {

int d3p_predict_confusion_set_strips(int32_t max_strips)
{
    if (max_strips == 0) max_strips = D3P_CONF_DEFAULT_STRIPS;
    if (max_strips < 1 || max_strips > 65535) return fail(D3P_E_INVALID_ARG, "d3p_predict_confusion_set_strips: 1 <= max_strips <= 65535 (0: the default)");
    g_conf_max_strips = (uint32_t)max_strips;
    return D3P_OK;
}

int d3p_predict_confusion(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows, int32_t d,
                          const float* latent_dev, int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n,
                          const uint32_t* obs_keys_dev, const float* tau_host, int32_t T, uint64_t* out_dev)
{
    const char* what = "d3p_predict_confusion";
    const d3p_logreg_model* m = model;
    if (int rc = validate_model(m, y_dev, what)) return rc;   // D3P_GUIDE_EXP_SITES: D3P_E_UNSUPPORTED
    if (m->family != D3P_FAMILY_LOGREG)
        return fail(D3P_E_UNSUPPORTED, "%s: logistic regression only (a confusion count needs 0 / 1 outcomes)", what);
    if (d != m->d) return fail(D3P_E_INVALID_ARG, "%s: d = %d differs from the model's %d", what, d, m->d);
    if (T < 0 || T > D3P_CONF_THRESHOLDS) return fail(D3P_E_INVALID_ARG, "%s: T = %d thresholds (0 <= T <= %d)", what, T, D3P_CONF_THRESHOLDS);
    if (T > 0 && !tau_host) return fail(D3P_E_INVALID_ARG, "%s: null tau pointer with T = %d", what, T);
    bool launch;
    if (int rc = glm_tile_check(what, m, rows, latent_ld, w_off, b_col, n, {X_dev, y_dev, latent_dev, obs_keys_dev, out_dev},
                                "X / y / latent / obs_keys / out", "X, y, latent, obs_keys and out", &launch))
        return rc;
    if (!launch) return fail(D3P_E_INVALID_ARG, "%s: rows must be >= 1 (a count over no rows says nothing)", what);
    if ((uintptr_t)y_dev % sizeof(float)) return fail(D3P_E_INVALID_ARG, "%s: y must be aligned to 4 bytes", what);
    if ((uintptr_t)out_dev % sizeof(uint64_t)) return fail(D3P_E_INVALID_ARG, "%s: out must be aligned to 8 bytes", what);
    ConfusionArgs g;
    g.tiles = cdiv(rows, D3P_TILE_N);
    g.per = (g.tiles + g_conf_max_strips - 1u) / g_conf_max_strips;
    const uint32_t strips = (g.tiles + g.per - 1u) / g.per;
    g.X = X_dev; g.y = y_dev; g.rows = rows; g.d = d; g.w_off = w_off; g.b_col = b_col; g.lat = latent_dev; g.ld = latent_ld; g.n = n;
    g.obs_keys = obs_keys_dev; g.out = reinterpret_cast<unsigned long long*>(out_dev);
    for (int j = 0; j < D3P_CONF_THRESHOLDS; ++j) g.tau[j] = j < T ? tau_host[j] : NAN;
    hipStream_t s = (hipStream_t)stream;
    D3P_HIP_TRY(hipMemsetAsync(out_dev, 0, sizeof(uint64_t) * D3P_CONF_COUNTS * (size_t)n, s));
    hipLaunchKernelGGL(k_predict_confusion, dim3(strips, cdiv(n, D3P_TILE_M)), dim3(256), 0, s, g);
    return check_launch(what);
}

size_t d3p_binary_curve_workspace(void) { return sizeof(uint64_t) * 2 * D3P_CURVE_CHUNKS; }

int d3p_binary_curve(void* stream, const float* p_dev, const int32_t* y_dev, uint64_t rows, uint32_t B, uint32_t* hist_dev, uint64_t* calib_dev,
                     uint64_t* summary_dev, void* workspace_dev, size_t workspace_bytes)
{
    const char* what = "d3p_binary_curve";
    if (!p_dev || !y_dev || !hist_dev || !calib_dev || !summary_dev || !workspace_dev)
        return fail(D3P_E_INVALID_ARG, "%s: null p / y / hist / calib / summary / workspace pointer", what);
    if (rows < 1) return fail(D3P_E_INVALID_ARG, "%s: rows must be >= 1 (a curve of no scores says nothing)", what);
    if (rows > (1ull << 27)) return fail(D3P_E_INVALID_ARG, "%s: rows <= 2^27 (the fixed-point sums of calib are exact up to there)", what);
    if (B < 1 || B > D3P_CURVE_MAX_CALIB) return fail(D3P_E_INVALID_ARG, "%s: B = %u reliability bins (1 <= B <= %d)", what, B, D3P_CURVE_MAX_CALIB);
    if ((uintptr_t)p_dev % 4 || (uintptr_t)y_dev % 4 || (uintptr_t)hist_dev % 4)
        return fail(D3P_E_INVALID_ARG, "%s: p, y and hist must be aligned to 4 bytes", what);
    if ((uintptr_t)calib_dev % 8 || (uintptr_t)summary_dev % 8 || (uintptr_t)workspace_dev % 8)
        return fail(D3P_E_INVALID_ARG, "%s: calib, summary and the workspace must be aligned to 8 bytes", what);
    if (workspace_bytes < d3p_binary_curve_workspace())
        return fail(D3P_E_INVALID_ARG, "%s: workspace of %zu bytes, %zu needed (d3p_binary_curve_workspace)", what, workspace_bytes,
                    d3p_binary_curve_workspace());
    for (const void* q : {(const void*)p_dev, (const void*)y_dev, (const void*)hist_dev, (const void*)calib_dev, (const void*)summary_dev,
                          (const void*)workspace_dev})
        if (!is_device_ptr(q)) return fail(D3P_E_INVALID_ARG, "%s: p, y, hist, calib, summary and the workspace must be device memory", what);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* calib = reinterpret_cast<unsigned long long*>(calib_dev);
    unsigned long long* summary = reinterpret_cast<unsigned long long*>(summary_dev);
    unsigned long long* chunk_tot = static_cast<unsigned long long*>(workspace_dev);
    D3P_HIP_TRY(hipMemsetAsync(hist_dev, 0, sizeof(uint32_t) * 2 * (size_t)D3P_CURVE_BINS, s));
    D3P_HIP_TRY(hipMemsetAsync(calib_dev, 0, sizeof(uint64_t) * 3 * (size_t)B, s));
    D3P_HIP_TRY(hipMemsetAsync(summary_dev, 0, sizeof(uint64_t) * D3P_CURVE_SUMMARY, s));
    const uint32_t blocks = cdiv(rows, 256) < 2048u ? cdiv(rows, 256) : 2048u;
    hipLaunchKernelGGL(k_curve_hist, dim3(blocks), dim3(256), 0, s, p_dev, y_dev, rows, B, hist_dev, calib, summary);
    if (int rc = check_launch(what)) return rc;
    hipLaunchKernelGGL(k_curve_chunks, dim3(D3P_CURVE_CHUNKS), dim3(256), 0, s, hist_dev, chunk_tot, summary);
    if (int rc = check_launch(what)) return rc;
    hipLaunchKernelGGL(k_curve_totals, dim3(D3P_CURVE_CHUNKS), dim3(256), 0, s, hist_dev, chunk_tot, summary);
    return check_launch(what);
}

}  // extern "C"
