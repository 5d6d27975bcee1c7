// Per-draw sums of the pointwise log-likelihood of the regression families over a whole table (d3p_amd/diagnostics.py: the full-data
// log joint, the ELBO and the Pareto k of a guide's importance ratios):
//   draw-sums form   out[s] = sum_{r < rows} ll[s, r]   as float64,   ll[s, r] = log p(y_r | t[s, r]),  t[s, r] = X[r] . w_s (+ b_s)
// ll[s, r] is bit for bit the float32 value the rows form (k_loglik, d3p_loglik.hip) writes: the same tile product, the same
// intercept add, the same label constant and the same loglik_value<FAMILY> (d3p_glm_tile.h).  Every other reduction over the tile
// (lppd, the moments, WAIC) runs over the draws, once per row; this one runs over the rows, once per draw.
//
// Grid: x = row strips, y = tiles of 128 draws.  The table's row tiles (128 rows) are cut into strips of `per` consecutive tiles by
// row_strips (d3p_row_sums.h, the definitions every per-draw reduction over rows shares),
//   tiles = ceil(rows / 128);  per = ceil(tiles / 512);  strips = ceil(tiles / per)  (<= 512)
// a function of rows alone -- not of the device, its CU count or n -- so the summation order below is a function of the arguments
// only.  A workgroup walks the row tiles of its strip in ascending order; X is read once per draw tile, as in the rows form.
//
// Epilogue, per half of a wave's 64 draws: the accumulators go through LDS as in the sibling kernels (tile_scatter: [draw 0..31]
// [row 0..63], rows padded to 65 floats), but here lane l takes DRAW l % 32 and the row half l / 32 of the wave's 64 rows and walks
// 32 rows at L[(l % 32) * 65 + 32 (l / 32) + j]: the 32 lanes of an LDS lane group read 32 distinct banks ((l % 32 + j) mod 32).
// y[r] and the label's constant (Poisson: lgammaf(y + 1), once per row as in the rows form) are staged in LDS once per row tile; all
// lanes of a group read the same element of them (a broadcast).  A lane keeps one float64 running sum per draw across the row tiles of
// the strip: sum += (double)ll, an IEEE float64 addition of the float32 value, nothing clamped (a -inf draw stays -inf, a NaN a NaN).
// Rows past `rows` are never evaluated (exp of a padded row's zero predictor is not 0), draws past n are never stored, and k >= d is
// staged as zeros by the tile.
//
// Summation order of out[s], fixed:  a tile's 128 rows fall into four quarters q = 0..3 of 32 consecutive rows.  Quarter sum (strip,
// q) = the rows of quarter q of every tile of the strip, tiles ascending, rows ascending within a tile, added one by one from 0.0.
// Strip partial = ((q0 + q1) + q2) + q3, written to the workspace as float64 [strip][n].  A second launch (k_strip_merge<1, -1, -1>, one
// thread per draw) adds the strips' partials in ascending strip order, starting from strip 0's.  No floating-point atomics, no
// arrival-order dependence: the output bits are a function of the arguments only.
#include "d3p_device.h"
#include "d3p_glm_tile.h"
#include "d3p_host.h"
#include "d3p_row_sums.h"

namespace d3p {

struct DrawSumsArgs {
    const float* X;
    const float* y;
    uint64_t rows;
    int d, w_off, b_col;
    const float* lat;
    int64_t ld;
    uint32_t n;
    float nh, ll_const;     // LINREG: -0.5 / sigma^2 and log sigma + log(2 pi) / 2, as the rows form gets them
    uint32_t tiles, per;    // row tiles of the table; row tiles per strip
    double* part;           // [strips][n]
};

// Registers: the X addresses of the staging loads live across the row-tile loop beside the 64 accumulators, as in k_loglik's lppd
// form, which spills at two waves per SIMD: one wave per SIMD, no scratch (docs/experiments_guide_diag.md).
template <int FAMILY>
__global__ void __launch_bounds__(256, 1) k_draw_sums(DrawSumsArgs g)
{
    // [k][draw] | [k][row] during the product; then each wave's t, half a tile at a time (4 x 32 x 65 floats); at the end 4 x 128 doubles
    __shared__ __attribute__((aligned(16))) float smem[D3P_TILE_SMEM];
    __shared__ float ys[D3P_TILE_N], cs[D3P_TILE_N];   // the row tile's labels and label constants
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int i = lane & 31, h = lane >> 5;            // the lane's draw within a half of the wave's draws; its half of the wave's rows
    const int col = wn * 64 + h * 32;                  // first of the lane's 32 rows within a tile: quarter q = 2 wn + h
    const uint32_t s0 = blockIdx.y * D3P_TILE_M;
    uint32_t t_lo, t_hi;
    strip_tiles(g.per, g.tiles, t_lo, t_hi);
    uint32_t s[2];
    float b[2];
    double sum[2] = {0.0, 0.0};
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        s[mb] = s0 + wm * 64 + mb * 32 + i;
        b[mb] = (g.b_col >= 0 && s[mb] < g.n) ? g.lat[(size_t)s[mb] * g.ld + g.b_col] : 0.f;
    }
    for (uint32_t t = t_lo; t < t_hi; ++t) {
        const uint64_t r0 = (uint64_t)t * D3P_TILE_N;
        if (tid < D3P_TILE_N) {   // (the product's barriers come between this and its readers; the last readers are behind a barrier)
            const uint64_t r = r0 + tid;
            const float y = r < g.rows ? g.y[r] : 0.f;
            ys[tid] = y;
            cs[tid] = FAMILY == D3P_FAMILY_POISSON ? lgammaf(y + 1.0f) : g.ll_const;
        }
        tile_f16v acc[2][2];
        tile_product(smem, g, r0, s0, acc);
        float* L = tile_block(smem);
        const int jn = quarter_live_rows(g.rows, r0, col);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            tile_scatter(L, acc[mb][0], acc[mb][1]);
            __syncthreads();
            if (s[mb] < g.n) {
                const float* p = L + i * 65 + h * 32;
                for (int j = 0; j < jn; ++j) {
                    float tv = p[j];
                    if (g.b_col >= 0) tv = tv + b[mb];
                    sum[mb] += (double)loglik_value<FAMILY>(tv, ys[col + j], g.nh, cs[col + j]);
                }
            }
            __syncthreads();
        }
    }
    // the four row quarters of a draw, merged in the order q = 0, 1, 2, 3 by the thread that owns the draw
    double* red = reinterpret_cast<double*>(smem);   // [q][draw of the tile]
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) red[(wn * 2 + h) * D3P_TILE_M + wm * 64 + mb * 32 + i] = sum[mb];
    __syncthreads();
    if (tid < D3P_TILE_M && s0 + tid < g.n) g.part[(size_t)blockIdx.x * g.n + s0 + tid] = quarter_sum(red + tid, D3P_TILE_M);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

size_t d3p_loglik_draw_sums_workspace(uint64_t rows, uint32_t n)
{
    uint32_t tiles, per, strips;
    row_strips(rows, D3P_TILE_N, D3P_ROW_SUMS_MAX_STRIPS, &tiles, &per, &strips);
    return (size_t)strips * n * sizeof(double);
}

int d3p_loglik_draw_sums(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows,
                         const float* latent_dev, int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, double* out_draws_dev,
                         void* workspace_dev, size_t workspace_bytes)
{
    const char* what = "d3p_loglik_draw_sums";
    const d3p_logreg_model* m = model;
    if (int rc = validate_model(m, y_dev, what)) return rc;   // D3P_GUIDE_EXP_SITES: D3P_E_UNSUPPORTED, as for the other forms
    bool launch;
    if (int rc = glm_tile_check(what, m, rows, latent_ld, w_off, b_col, n, {X_dev, y_dev, latent_dev, out_draws_dev}, "X / y / latent / out",
                                "X, y, latent and out", &launch))
        return rc;
    if ((uintptr_t)out_draws_dev % sizeof(double)) return fail(D3P_E_INVALID_ARG, "%s: out must be aligned to 8 bytes", what);
    hipStream_t s = (hipStream_t)stream;
    if (!launch) {   // rows == 0: the empty sum, without a launch
        if (!is_device_ptr(out_draws_dev)) return fail(D3P_E_INVALID_ARG, "%s: out must be device memory", what);
        D3P_HIP_TRY(hipMemsetAsync(out_draws_dev, 0, (size_t)n * sizeof(double), s));
        return D3P_OK;
    }
    DrawSumsArgs g;
    uint32_t strips;
    row_strips(rows, D3P_TILE_N, D3P_ROW_SUMS_MAX_STRIPS, &g.tiles, &g.per, &strips);
    if (int rc = row_workspace_check(what, "d3p_loglik_draw_sums_workspace", workspace_dev, workspace_bytes, strips, 1, n)) return rc;
    g.X = X_dev; g.y = y_dev; g.rows = rows; g.d = m->d; g.w_off = w_off; g.b_col = b_col; g.lat = latent_dev; g.ld = latent_ld; g.n = n;
    g.part = static_cast<double*>(workspace_dev);
    // as the rows form's arguments (d3p_loglik.hip)
    const bool sigma = m->family == D3P_FAMILY_LINREG;
    g.nh = sigma ? -0.5f / (m->lik_sigma * m->lik_sigma) : 0.f;
    g.ll_const = sigma ? logf(m->lik_sigma) + 0.91893853320467267f : 0.f;
    const dim3 grid(strips, cdiv(n, D3P_TILE_M));
    if (m->family == D3P_FAMILY_LINREG) hipLaunchKernelGGL((k_draw_sums<D3P_FAMILY_LINREG>), grid, dim3(256), 0, s, g);
    else if (m->family == D3P_FAMILY_POISSON) hipLaunchKernelGGL((k_draw_sums<D3P_FAMILY_POISSON>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((k_draw_sums<D3P_FAMILY_LOGREG>), grid, dim3(256), 0, s, g);
    if (int rc = check_launch(what)) return rc;
    return strip_merge<1, -1, -1>(what, s, g.part, strips, n, out_draws_dev);
}

}  // extern "C"
