// Per-draw statistics of a replicated data set over its ROWS (d3p_amd/ppc.py: posterior predictive checks).
// For draw s over the values v[s, r], r < rows (float32 or int32, taken to float64 exactly) and a host-given float64 shift c:
//   out[0 n + s] = sum_r e,  e = fl64(v - c)          out[1 n + s] = sum_r fl64(e e)   (product and addition: two roundings)
//   out[2 n + s] = min_r v   out[3 n + s] = max_r v   out[4 n + s] = #{r : v == 0}     (-0.0 counts, NaN does not)
// Two forms with ONE accumulation (rep_add), one quarter merge (rep_strip_partial) and one strip merge (k_strip_merge<5, 2, 3>):
//   k_rep_stats<T>           v is a matrix in memory, m[s ld + r]                          (d3p_rep_stats)
//   k_predict_stats<FAMILY>  v is the outcome the predictive kernels WOULD store, bit for bit: the shared product tile, the same
//                            intercept add, the same outcome rule (d3p_outcome.h, normal_site_value) with the same obs keys, rows
//                            and r as k_predict_glm / k_predict_logreg -- the n x rows matrix is never written  (d3p_predict_stats)
//
// Summation order of outputs 0 and 1: d3p_loglik_draw_sums' (d3p_draw_sums.hip), a function of the arguments alone -- the same
// row_strips, strip_tiles, quarter_sum and k_strip_merge (d3p_row_sums.h).
//   tiles = ceil(rows / 128);  per = ceil(tiles / 512);  strips = ceil(tiles / per)
// A tile's 128 rows fall into four quarters of 32 consecutive rows.  One accumulator per (draw, strip, quarter) runs over the
// strip's tiles ascending and rows ascending from 0.0; strip partial = ((q0 + q1) + q2) + q3, written to the workspace as float64
// [strip][5][n]; the merge launch adds the strips in ascending order starting from strip 0's.  No floating-point atomics.  min, max and
// the zero count are kept in 32-bit registers (exact in float64 afterwards) and merged by value; a NaN sets a flag per accumulator
// (fminf alone would drop it) that turns min and max into NaN, and outputs 0 and 1 are NaN by arithmetic.  Nothing is clamped.
//
// k_rep_stats: grid (strips, tiles of 128 draws), 4 waves.  Per row tile and half of the draw tile, wave w stages draws 16 w .. 16 w +
// 15: one wave-load is 64 consecutive rows of a draw (256 contiguous bytes), two of them the 128 rows of the tile, into LDS [draw
// 0..63][row 0..127] with rows padded to 129 words.  Then wave q = quarter, lane = draw: lane l walks 32 rows at L[l 129 + 32 q + j],
// 64 lanes on 64 distinct banks ((l + j) mod 64).
// k_predict_stats: k_draw_sums' grid and epilogue (lane = draw l % 32 and row half l / 32 of the wave's 64 rows, walking 32 rows on 32
// distinct banks), the per-draw keys in LDS once per workgroup (stage_obs_keys, d3p_outcome.h).  The draw halves are NOT unrolled (the
// outcome rule, glm_outcome, Poisson's above all, is instantiated once); the lane's two accumulators are picked by hand, so nothing is
// indexed in scratch.
#include "d3p_device.h"
#include "d3p_glm_tile.h"
#include "d3p_host.h"
#include "d3p_outcome.h"
#include "d3p_row_sums.h"

namespace d3p {

#define D3P_REP_STATS 5
#define D3P_REP_LD 129           // padded row count of a staged draw (k_rep_stats)
#define D3P_REP_HALF 64          // draws staged at a time (k_rep_stats)

// one (draw, strip, quarter) accumulator; T = float or int32_t
template <class T>
struct RepAcc {
    double sum, sq;
    T mn, mx;
    uint32_t zeros, nan;
};

template <class T> __device__ __forceinline__ T rep_lowest();
template <class T> __device__ __forceinline__ T rep_highest();
template <> __device__ __forceinline__ float rep_lowest<float>() { return -INFINITY; }
template <> __device__ __forceinline__ float rep_highest<float>() { return INFINITY; }
template <> __device__ __forceinline__ int32_t rep_lowest<int32_t>() { return (int32_t)0x80000000; }
template <> __device__ __forceinline__ int32_t rep_highest<int32_t>() { return 0x7fffffff; }

template <class T>
__device__ __forceinline__ void rep_init(RepAcc<T>& a)
{
    a.sum = 0.0; a.sq = 0.0; a.mn = rep_highest<T>(); a.mx = rep_lowest<T>(); a.zeros = 0u; a.nan = 0u;
}

// THE accumulation of both forms: e = fl64(v - c); sum += e; sq += fl64(e e) -- the product is rounded before the addition
template <class T>
__device__ __forceinline__ void rep_add(RepAcc<T>& a, T v, double c)
{
#pragma clang fp contract(off)
    const double e = (double)v - c;
    const double ee = e * e;
    a.sum = a.sum + e;
    a.sq = a.sq + ee;
    a.mn = v < a.mn ? v : a.mn;
    a.mx = v > a.mx ? v : a.mx;
    a.zeros += v == (T)0 ? 1u : 0u;
    a.nan |= v != v ? 1u : 0u;   // (int32: never)
}

// red: [stat][quarter][draw of the tile] float64, 5 x 4 x 128
template <class T>
__device__ __forceinline__ void rep_put(double* red, int q, int dl, const RepAcc<T>& a)
{
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    red[(0 * 4 + q) * D3P_TILE_M + dl] = a.sum;
    red[(1 * 4 + q) * D3P_TILE_M + dl] = a.sq;
    red[(2 * 4 + q) * D3P_TILE_M + dl] = a.nan ? nanv : (double)a.mn;
    red[(3 * 4 + q) * D3P_TILE_M + dl] = a.nan ? nanv : (double)a.mx;
    red[(4 * 4 + q) * D3P_TILE_M + dl] = (double)a.zeros;
}

// the four quarters of draw dl in the order q = 0, 1, 2, 3 -> part[strip][stat][n]; called by the threads dl < 128 after a barrier
// (min and max by rep_min / rep_max, d3p_row_sums.h: a NaN is carried)
__device__ __forceinline__ void rep_strip_partial(const double* red, int dl, uint32_t s, uint32_t n, uint32_t strip, double* part)
{
    const int M = D3P_TILE_M;
    const double* r = red + dl;
    double* p = part + (size_t)strip * D3P_REP_STATS * n + s;
    p[0] = quarter_sum(r, M);
    p[n] = quarter_sum(r + 4 * M, M);
    r += 8 * M;
    p[2 * (size_t)n] = rep_min(rep_min(rep_min(r[0], r[M]), r[2 * M]), r[3 * M]);
    r += 4 * M;
    p[3 * (size_t)n] = rep_max(rep_max(rep_max(r[0], r[M]), r[2 * M]), r[3 * M]);
    p[4 * (size_t)n] = quarter_sum(r + 4 * M, M);   // (counts: exact)
}

// ---- the model-free form ---------------------------------------------------------------------------------------------------------
struct RepStatsArgs {
    const void* m;
    int64_t ld;
    uint32_t n;
    uint64_t rows;
    double shift;
    uint32_t tiles, per;
    double* part;   // [strips][5][n]
};

template <class T>
__global__ void __launch_bounds__(256) k_rep_stats(RepStatsArgs g)
{
    // the staged half tile [64 draws][129]; at the end 5 x 4 x 128 doubles
    __shared__ __attribute__((aligned(16))) T smem[D3P_REP_HALF * D3P_REP_LD];
    static_assert(sizeof(T) * D3P_REP_HALF * D3P_REP_LD >= sizeof(double) * D3P_REP_STATS * 4 * D3P_TILE_M, "the quarter merge fits");
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;   // q: the wave, and the quarter it walks
    const T* m = static_cast<const T*>(g.m);
    const uint32_t s0 = blockIdx.y * D3P_TILE_M;
    uint32_t t_lo, t_hi;
    strip_tiles(g.per, g.tiles, t_lo, t_hi);
    const int col = q * 32;
    RepAcc<T> acc[2];
    rep_init(acc[0]);
    rep_init(acc[1]);
    for (uint32_t t = t_lo; t < t_hi; ++t) {
        const uint64_t r0 = (uint64_t)t * D3P_TILE_N;
        const uint64_t left = g.rows - r0;   // >= 1: the tile's live rows, for the staging
        const int jn = quarter_live_rows(g.rows, r0, col);
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int dl = q * 16 + k;
                const uint32_t s = s0 + hb * D3P_REP_HALF + dl;
                if (s < g.n) {
                    const T* src = m + (size_t)s * g.ld + r0;
                    if ((uint64_t)lane < left) smem[dl * D3P_REP_LD + lane] = src[lane];
                    if ((uint64_t)lane + 64 < left) smem[dl * D3P_REP_LD + 64 + lane] = src[lane + 64];
                }
            }
            __syncthreads();
            if (s0 + hb * D3P_REP_HALF + lane < g.n) {
                const T* p = smem + lane * D3P_REP_LD + col;
                for (int j = 0; j < jn; ++j) rep_add(acc[hb], p[j], g.shift);
            }
            __syncthreads();
        }
    }
    double* red = reinterpret_cast<double*>(smem);
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) rep_put(red, q, hb * D3P_REP_HALF + lane, acc[hb]);
    __syncthreads();
    if (tid < D3P_TILE_M && s0 + tid < g.n) rep_strip_partial(red, tid, s0 + tid, g.n, blockIdx.x, g.part);
}

// ---- the fused form --------------------------------------------------------------------------------------------------------------
struct PredictStatsArgs {
    const float* X;
    uint64_t rows;
    int d, w_off, b_col;
    const float* lat;
    int64_t ld;
    uint32_t n;
    float sigma;   // LINREG: the observation's standard deviation
    const uint32_t* obs_keys;
    double shift;
    uint32_t tiles, per;
    double* part;   // [strips][5][n]
};

template <int FAMILY> struct rep_value { typedef int32_t type; };
template <> struct rep_value<D3P_FAMILY_LINREG> { typedef float type; };

// Registers: one wave per SIMD as k_draw_sums (the X addresses of the staging loads live across the row-tile loop beside the 64
// accumulators); the figures of the three instantiations: docs/experiments_ppc.md
template <int FAMILY>
__global__ void __launch_bounds__(256, 1) k_predict_stats(PredictStatsArgs g)
{
    typedef typename rep_value<FAMILY>::type T;
    // [k][draw] | [k][row] during the product; then each wave's t, half a tile at a time (4 x 32 x 65 floats); at the end 5 x 4 x 128 doubles
    __shared__ __attribute__((aligned(16))) float smem[D3P_TILE_SMEM];
    static_assert(sizeof(float) * D3P_TILE_SMEM >= sizeof(double) * D3P_REP_STATS * 4 * D3P_TILE_M, "the quarter merge fits");
    __shared__ uint32_t keys[D3P_TILE_M][4];   // per draw of the tile: the obs key and fold_in(obs key, 0)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int i = lane & 31, h = lane >> 5;            // the lane's draw within a half of the wave's draws; its half of the wave's rows
    const int col = wn * 64 + h * 32;                  // first of the lane's 32 rows within a tile: quarter q = 2 wn + h
    const uint32_t s0 = blockIdx.y * D3P_TILE_M;
    uint32_t t_lo, t_hi;
    strip_tiles(g.per, g.tiles, t_lo, t_hi);
    stage_obs_keys<FAMILY>(keys, g.obs_keys, s0, g.n);
    RepAcc<T> a0, a1;
    rep_init(a0);
    rep_init(a1);
    for (uint32_t t = t_lo; t < t_hi; ++t) {
        const uint64_t r0 = (uint64_t)t * D3P_TILE_N;
        tile_f16v acc[2][2];
        tile_product(smem, g, r0, s0, acc);
        float* L = tile_block(smem);
        const int jn = quarter_live_rows(g.rows, r0, col);
#pragma unroll 1
        for (int mb = 0; mb < 2; ++mb) {
            tile_scatter(L, mb == 0 ? acc[0][0] : acc[1][0], mb == 0 ? acc[0][1] : acc[1][1]);   // (selected by hand: the loop is not unrolled)
            __syncthreads();
            const int sl = wm * 64 + mb * 32 + i;
            const uint32_t s = s0 + sl;
            if (s < g.n) {
                RepAcc<T> a = mb == 0 ? a0 : a1;
                const float b = g.b_col >= 0 ? g.lat[(size_t)s * g.ld + g.b_col] : 0.f;
                const uint32_t o0 = keys[sl][0], o1 = keys[sl][1];
                const float* p = L + i * 65 + h * 32;
                const uint64_t rb = r0 + col;
#pragma unroll 1
                for (int j = 0; j < jn; ++j) {
                    float tv = p[j];
                    if (g.b_col >= 0) tv = tv + b;
                    const T v = glm_outcome<FAMILY>(tv, o0, o1, keys[sl][2], keys[sl][3], g.rows, rb + j, g.sigma);
                    rep_add(a, v, g.shift);
                }
                if (mb == 0) a0 = a; else a1 = a;
            }
            __syncthreads();
        }
    }
    double* red = reinterpret_cast<double*>(smem);   // [stat][q][draw of the tile]
    rep_put(red, wn * 2 + h, wm * 64 + i, a0);
    rep_put(red, wn * 2 + h, wm * 64 + 32 + i, a1);
    __syncthreads();
    if (tid < D3P_TILE_M && s0 + tid < g.n) rep_strip_partial(red, tid, s0 + tid, g.n, blockIdx.x, g.part);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

size_t d3p_rep_stats_workspace(uint64_t rows, uint32_t n)
{
    if (rows > 0xFFFFFFFFull) return 0;
    uint32_t tiles, per, strips;
    row_strips(rows, D3P_TILE_N, D3P_ROW_SUMS_MAX_STRIPS, &tiles, &per, &strips);
    return (size_t)strips * D3P_REP_STATS * n * sizeof(double);
}

int d3p_rep_stats(void* stream, const void* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t rows, double shift, double* out_dev,
                  void* workspace_dev, size_t workspace_bytes)
{
    const char* what = "d3p_rep_stats";
    if (!m_dev || !out_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((uintptr_t)m_dev % 4 || (uintptr_t)out_dev % sizeof(double))
        return fail(D3P_E_INVALID_ARG, "%s: the matrix must be aligned to 4 bytes, out to 8", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n must be >= 1", what);
    if (rows == 0) return fail(D3P_E_INVALID_ARG, "%s: rows must be >= 1 (the minimum and maximum of nothing are undefined)", what);
    if (rows > 0xFFFFFFFFull || cdiv(n, D3P_TILE_M) > 65535u) return fail(D3P_E_UNSUPPORTED, "%s: rows < 2^32 and n <= 128 x 65535", what);
    if (ld < 0 || (uint64_t)ld < rows) return fail(D3P_E_INVALID_ARG, "%s: ld >= rows is required", what);
    if (!std::isfinite(shift)) return fail(D3P_E_INVALID_ARG, "%s: the shift must be finite", what);
    RepStatsArgs g;
    uint32_t strips;
    row_strips(rows, D3P_TILE_N, D3P_ROW_SUMS_MAX_STRIPS, &g.tiles, &g.per, &strips);
    if (int rc = row_workspace_check(what, "d3p_rep_stats_workspace", workspace_dev, workspace_bytes, strips, D3P_REP_STATS, n)) return rc;
    if (!is_device_ptr(m_dev) || !is_device_ptr(out_dev)) return fail(D3P_E_INVALID_ARG, "%s: the matrix and out must be device memory", what);
    g.m = m_dev; g.ld = ld; g.n = n; g.rows = rows; g.shift = shift; g.part = static_cast<double*>(workspace_dev);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(strips, cdiv(n, D3P_TILE_M));
    if (dtype == 0) hipLaunchKernelGGL((k_rep_stats<float>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((k_rep_stats<int32_t>), grid, dim3(256), 0, s, g);
    if (int rc = check_launch(what)) return rc;
    return strip_merge<D3P_REP_STATS, 2, 3>(what, s, g.part, strips, n, out_dev);
}

int d3p_predict_stats(void* stream, const d3p_logreg_model* model, const float* X_dev, uint64_t rows, int32_t d, const float* latent_dev,
                      int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, const uint32_t* obs_keys_dev, double shift,
                      double* out_dev, void* workspace_dev, size_t workspace_bytes)
{
    const char* what = "d3p_predict_stats";
    const d3p_logreg_model* m = model;
    // (there are no labels: validate_model's label check gets a pointer that is not null)
    if (int rc = validate_model(m, m, what)) return rc;   // D3P_GUIDE_EXP_SITES: D3P_E_UNSUPPORTED; LINREG: lik_sigma finite and > 0
    if (m->family != D3P_FAMILY_GAUSS_MEAN && d != m->d) return fail(D3P_E_INVALID_ARG, "%s: d = %d differs from the model's %d", what, d, m->d);
    if (m->family == D3P_FAMILY_POISSON && 2 * rows > 0xFFFFFFFFull)
        return fail(D3P_E_INVALID_ARG, "%s: Poisson outcomes need 2 rows < 2^32 (one threefry stream of 2 rows uniforms per iteration)", what);
    bool launch;
    if (int rc = glm_tile_check(what, m, rows, latent_ld, w_off, b_col, n, {X_dev, latent_dev, obs_keys_dev, out_dev}, "X / latent / obs_keys / out",
                                "X, latent, obs_keys and out", &launch))
        return rc;
    if (!launch) return fail(D3P_E_INVALID_ARG, "%s: rows must be >= 1 (the minimum and maximum of nothing are undefined)", what);
    if ((uintptr_t)out_dev % sizeof(double)) return fail(D3P_E_INVALID_ARG, "%s: out must be aligned to 8 bytes", what);
    if (!std::isfinite(shift)) return fail(D3P_E_INVALID_ARG, "%s: the shift must be finite", what);
    PredictStatsArgs g;
    uint32_t strips;
    row_strips(rows, D3P_TILE_N, D3P_ROW_SUMS_MAX_STRIPS, &g.tiles, &g.per, &strips);
    if (int rc = row_workspace_check(what, "d3p_rep_stats_workspace", workspace_dev, workspace_bytes, strips, D3P_REP_STATS, n)) return rc;
    g.X = X_dev; g.rows = rows; g.d = d; g.w_off = w_off; g.b_col = b_col; g.lat = latent_dev; g.ld = latent_ld; g.n = n;
    g.sigma = m->family == D3P_FAMILY_LINREG ? m->lik_sigma : 0.f;
    g.obs_keys = obs_keys_dev; g.shift = shift; g.part = static_cast<double*>(workspace_dev);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(strips, cdiv(n, D3P_TILE_M));
    if (m->family == D3P_FAMILY_LINREG) hipLaunchKernelGGL((k_predict_stats<D3P_FAMILY_LINREG>), grid, dim3(256), 0, s, g);
    else if (m->family == D3P_FAMILY_POISSON) hipLaunchKernelGGL((k_predict_stats<D3P_FAMILY_POISSON>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((k_predict_stats<D3P_FAMILY_LOGREG>), grid, dim3(256), 0, s, g);
    if (int rc = check_launch(what)) return rc;
    return strip_merge<D3P_REP_STATS, 2, 3>(what, s, g.part, strips, n, out_dev);
}

}  // extern "C"
