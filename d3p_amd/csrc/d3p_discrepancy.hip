// Realized-discrepancy sums of a fitted regression model over its ROWS (d3p_amd/discrepancy.py: the chi-square check of Gelman, Meng &
// Stern 1996 and the Bayesian R^2 of Gelman, Goodrich, Gabry & Vehtari 2019).  The one reduction over the rows that
// needs the observed y, the conditional mean mu and the replicated outcome v together.  For draw s and row r, t = the product tile's
// value (+ the intercept), as for every user of the tile:
//   mu = the float32 mean d3p_predict_mean_rows stores: k_mean_rows' link, glm_mean<FAMILY> (d3p_glm_tile.h)
//   v  = the outcome d3p_predict_glm / d3p_predict_logreg store: the same rule (glm_outcome, d3p_outcome.h), obs keys, rows and r
// and in float64, every operation rounded once (the file is compiled with fp contract off):
//   M = fl64(mu)     V = fl64(sigma) fl64(sigma) (linear) | M (Poisson) | M (1.0 - M) (logistic)
//   q(x) = (e == 0.0) ? 0.0 : (e e) / V,  e = fl64(x) - M          m = M - shift          ey = fl64(y_r) - M
//   out[0 n + s] = sum_r q(y_r)     out[1 n + s] = sum_r q(v[s, r])     out[2 n + s] = sum_r m     out[3 n + s] = sum_r fl64(m m)
//   out[4 n + s] = sum_r ey         out[5 n + s] = sum_r fl64(ey ey)
// ONE convention: a row that is matched exactly contributes nothing, even at V == 0; otherwise nothing is clamped (e != 0 at V == 0:
// +inf; a NaN mu: NaN; Poisson's markers -1 and 2147483647 are values like any other).
//
// Summation order of all six: d3p_rep_stats' (d3p_rep_stats.hip), which is d3p_loglik_draw_sums' (DESIGN.md section 4j), by the same
// definitions (d3p_row_sums.h: row_strips, strip_tiles, quarter_sum, k_strip_merge):
//   tiles = ceil(rows / 128);  per = ceil(tiles / 512);  strips = ceil(tiles / per)
// four quarter accumulators of 32 consecutive rows per tile, tiles and rows ascending from 0.0; strip partial = ((q0 + q1) + q2) + q3
// into the workspace as float64 [strip][6][n]; k_strip_merge<6, -1, -1> adds them ascending from strip 0's.  No floating-point atomics.
//
// k_predict_discrepancy<FAMILY> has k_predict_stats' shape: grid (row strips, tiles of 128 draws), tile_product per row tile,
// tile_scatter per draw half under `unroll 1`, lane = draw l % 32 and row half l / 32 walking 32 rows on 32 distinct LDS banks, the
// per-draw keys (and fold_in(obs key, 0) for Poisson) in LDS once per workgroup, the tile's 128 y values in LDS once per row tile (a
// lane group reads one element: a broadcast), the lane's two accumulator sets picked by hand.  ONE launch computes all six sums for
// every family: the Poisson form fills the register file of one wave per SIMD (256 VGPR + 256 AGPR) without scratch, and a form with the
// outcome rule and output 1 alone was no lighter (the figures and the decision: docs/experiments_discrepancy.md).
#include "d3p_device.h"
#include "d3p_glm_tile.h"
#include "d3p_host.h"
#include "d3p_outcome.h"
#include "d3p_row_sums.h"

#pragma clang fp contract(off)

namespace d3p {

#define D3P_DISC_SUMS 6

// q(x) = (e == 0.0) ? 0.0 : (e e) / V: an exactly matched row contributes nothing, even at V == 0; nothing else is clamped
__device__ __forceinline__ double disc_q(double e, double V) { return e == 0.0 ? 0.0 : (e * e) / V; }

// one (draw, strip, quarter) accumulator set
struct DiscAcc {
    double d_obs, d_rep, m1, m2, e1, e2;
};

__device__ __forceinline__ void disc_init(DiscAcc& a) { a.d_obs = 0.0; a.d_rep = 0.0; a.m1 = 0.0; a.m2 = 0.0; a.e1 = 0.0; a.e2 = 0.0; }

// red: [sum][quarter][draw of the tile] float64, 6 x 4 x 128
__device__ __forceinline__ void disc_put(double* red, int q, int dl, const DiscAcc& a)
{
    red[(0 * 4 + q) * D3P_TILE_M + dl] = a.d_obs;
    red[(1 * 4 + q) * D3P_TILE_M + dl] = a.d_rep;
    red[(2 * 4 + q) * D3P_TILE_M + dl] = a.m1;
    red[(3 * 4 + q) * D3P_TILE_M + dl] = a.m2;
    red[(4 * 4 + q) * D3P_TILE_M + dl] = a.e1;
    red[(5 * 4 + q) * D3P_TILE_M + dl] = a.e2;
}

struct DiscrepancyArgs {
    const float* X;
    const float* y;
    uint64_t rows;
    int d, w_off, b_col;
    const float* lat;
    int64_t ld;
    uint32_t n;
    float sigma;     // LINREG: the observation's standard deviation
    double var;      // LINREG: fl64(sigma) fl64(sigma)
    const uint32_t* obs_keys;
    double shift;
    uint32_t tiles, per;
    double* part;    // [strips][6][n]
};

// Registers: one wave per SIMD as k_predict_stats; the figures of every instantiation: docs/experiments_discrepancy.md
template <int FAMILY>
__global__ void __launch_bounds__(256, 1) k_predict_discrepancy(DiscrepancyArgs g)
{
    // [k][draw] | [k][row] during the product; then each wave's t, half a tile at a time (4 x 32 x 65 floats); at the end 6 x 4 x 128 doubles
    __shared__ __attribute__((aligned(16))) float smem[D3P_TILE_SMEM];
    static_assert(sizeof(float) * D3P_TILE_SMEM >= sizeof(double) * D3P_DISC_SUMS * 4 * D3P_TILE_M, "the quarter merge fits");
    __shared__ uint32_t keys[D3P_TILE_M][4];   // per draw of the tile: the obs key and fold_in(obs key, 0)
    __shared__ float ys[D3P_TILE_N];           // the row tile's observed outcomes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int i = lane & 31, h = lane >> 5;            // the lane's draw within a half of the wave's draws; its half of the wave's rows
    const int col = wn * 64 + h * 32;                  // first of the lane's 32 rows within a tile: quarter q = 2 wn + h
    const uint32_t s0 = blockIdx.y * D3P_TILE_M;
    uint32_t t_lo, t_hi;
    strip_tiles(g.per, g.tiles, t_lo, t_hi);
    stage_obs_keys<FAMILY>(keys, g.obs_keys, s0, g.n);
    DiscAcc a0, a1;
    disc_init(a0);
    disc_init(a1);
    for (uint32_t t = t_lo; t < t_hi; ++t) {
        const uint64_t r0 = (uint64_t)t * D3P_TILE_N;
        if (tid < D3P_TILE_N) {   // (the product's barriers come between this and its readers; the last readers are behind a barrier)
            const uint64_t r = r0 + tid;
            ys[tid] = r < g.rows ? g.y[r] : 0.f;
        }
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
                DiscAcc a = mb == 0 ? a0 : a1;
                const float b = g.b_col >= 0 ? g.lat[(size_t)s * g.ld + g.b_col] : 0.f;
                const uint32_t o0 = keys[sl][0], o1 = keys[sl][1];
                const float* p = L + i * 65 + h * 32;
                const uint64_t rb = r0 + col;
#pragma unroll 1
                for (int j = 0; j < jn; ++j) {
                    float tv = p[j];
                    if (g.b_col >= 0) tv = tv + b;
                    const double M = (double)glm_mean<FAMILY>(tv);
                    const double V = FAMILY == D3P_FAMILY_LINREG ? g.var : (FAMILY == D3P_FAMILY_POISSON ? M : M * (1.0 - M));
                    const double m = M - g.shift;
                    const double ey = (double)ys[col + j] - M;
                    a.d_obs = a.d_obs + disc_q(ey, V);
                    a.m1 = a.m1 + m;
                    a.m2 = a.m2 + m * m;
                    a.e1 = a.e1 + ey;
                    a.e2 = a.e2 + ey * ey;
                    const double v = (double)glm_outcome<FAMILY>(tv, o0, o1, keys[sl][2], keys[sl][3], g.rows, rb + j, g.sigma);
                    a.d_rep = a.d_rep + disc_q(v - M, V);
                }
                if (mb == 0) a0 = a; else a1 = a;
            }
            __syncthreads();
        }
    }
    double* red = reinterpret_cast<double*>(smem);   // [sum][q][draw of the tile]
    disc_put(red, wn * 2 + h, wm * 64 + i, a0);
    disc_put(red, wn * 2 + h, wm * 64 + 32 + i, a1);
    __syncthreads();
    if (tid < D3P_TILE_M && s0 + tid < g.n) {   // the four quarters of draw tid in the order q = 0, 1, 2, 3 -> part[strip][sum][n]
        double* p = g.part + (size_t)blockIdx.x * D3P_DISC_SUMS * g.n + s0 + tid;
#pragma unroll
        for (int k = 0; k < D3P_DISC_SUMS; ++k) p[k * (size_t)g.n] = quarter_sum(red + k * 4 * D3P_TILE_M + tid, D3P_TILE_M);
    }
}

}  // namespace d3p

using namespace d3p;

extern "C" {

size_t d3p_predict_discrepancy_workspace(uint64_t rows, uint32_t n)
{
    if (rows > 0xFFFFFFFFull) return 0;
    uint32_t tiles, per, strips;
    row_strips(rows, D3P_TILE_N, D3P_ROW_SUMS_MAX_STRIPS, &tiles, &per, &strips);
    return (size_t)strips * D3P_DISC_SUMS * n * sizeof(double);
}

int d3p_predict_discrepancy(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows, int32_t d,
                            const float* latent_dev, int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n,
                            const uint32_t* obs_keys_dev, double shift, double* out_dev, void* workspace_dev, size_t workspace_bytes)
{
    const char* what = "d3p_predict_discrepancy";
    const d3p_logreg_model* m = model;
    if (int rc = validate_model(m, y_dev, what)) return rc;   // D3P_GUIDE_EXP_SITES: D3P_E_UNSUPPORTED; LINREG: lik_sigma finite and > 0
    if (m->family != D3P_FAMILY_GAUSS_MEAN && d != m->d) return fail(D3P_E_INVALID_ARG, "%s: d = %d differs from the model's %d", what, d, m->d);
    if (m->family == D3P_FAMILY_POISSON && 2 * rows > 0xFFFFFFFFull)
        return fail(D3P_E_INVALID_ARG, "%s: Poisson outcomes need 2 rows < 2^32 (one threefry stream of 2 rows uniforms per iteration)", what);
    bool launch;
    if (int rc = glm_tile_check(what, m, rows, latent_ld, w_off, b_col, n, {X_dev, y_dev, latent_dev, obs_keys_dev, out_dev},
                                "X / y / latent / obs_keys / out", "X, y, latent, obs_keys and out", &launch))
        return rc;
    if (!launch) return fail(D3P_E_INVALID_ARG, "%s: rows must be >= 1 (a discrepancy over no rows says nothing)", what);
    if ((uintptr_t)y_dev % sizeof(float)) return fail(D3P_E_INVALID_ARG, "%s: y must be aligned to 4 bytes", what);
    if ((uintptr_t)out_dev % sizeof(double)) return fail(D3P_E_INVALID_ARG, "%s: out must be aligned to 8 bytes", what);
    if (!std::isfinite(shift)) return fail(D3P_E_INVALID_ARG, "%s: the shift must be finite", what);
    DiscrepancyArgs g;
    uint32_t strips;
    row_strips(rows, D3P_TILE_N, D3P_ROW_SUMS_MAX_STRIPS, &g.tiles, &g.per, &strips);
    if (int rc = row_workspace_check(what, "d3p_predict_discrepancy_workspace", workspace_dev, workspace_bytes, strips, D3P_DISC_SUMS, n)) return rc;
    g.X = X_dev; g.y = y_dev; g.rows = rows; g.d = d; g.w_off = w_off; g.b_col = b_col; g.lat = latent_dev; g.ld = latent_ld; g.n = n;
    g.sigma = m->family == D3P_FAMILY_LINREG ? m->lik_sigma : 0.f;
    g.var = (double)g.sigma * (double)g.sigma;
    g.obs_keys = obs_keys_dev; g.shift = shift; g.part = static_cast<double*>(workspace_dev);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(strips, cdiv(n, D3P_TILE_M));
    if (m->family == D3P_FAMILY_LINREG) hipLaunchKernelGGL((k_predict_discrepancy<D3P_FAMILY_LINREG>), grid, dim3(256), 0, s, g);
    else if (m->family == D3P_FAMILY_POISSON) hipLaunchKernelGGL((k_predict_discrepancy<D3P_FAMILY_POISSON>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((k_predict_discrepancy<D3P_FAMILY_LOGREG>), grid, dim3(256), 0, s, g);
    if (int rc = check_launch(what)) return rc;
    return strip_merge<D3P_DISC_SUMS, -1, -1>(what, s, g.part, strips, n, out_dev);
}

}  // extern "C"
