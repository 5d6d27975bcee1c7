// Posterior predictive mean and variance of the regression families over posterior draws (d3p_amd/prediction.py): the moments of
// the mixture (1/n) sum_s p(y | x_r, w_s, b_s), from the families' closed-form conditional moments -- no outcome is sampled.
//   t[s, r]  = X[r] . w_s (+ b_s)
//   mu[s, r] = E[y | t]:    sigmoid(t)   | t        | exp(t)              (logistic | linear | Poisson)
//   v[s, r]  = Var[y | t]:  mu (1 - mu)  | sigma^2  | mu
//   mean[r]  = (1/n) sum_s mu[s, r]
//   var[r]   = (1/n) sum_s v[s, r] + (1/n) sum_s (mu[s, r] - mean[r])^2      (law of total variance, population form)
//
// The product is the shared tile (d3p_glm_tile.h): 128 draws x 128 rows per workgroup, 4 wavefronts (2 x 2: wm = draw half, wn = row
// half) of 64 x 64; as in k_loglik's lppd form (d3p_loglik.hip) the grid runs over row tiles only and the workgroup walks the draw
// tiles; the accumulators go through LDS so that lane l owns row l and walks 32 draws.
//
// Epilogue in float32, no clamps (exp(t) = inf stays inf); accumulation per lane and row, in draw order, in float64:
//   logistic          sum p and sum q, p = sigmoid(t) and q = sigmoid(-t) both formed from ONE e = exp(-|t|) (the smaller is
//                     e / (1 + e), the larger 1 / (1 + e): neither is 1 - the other); mean = P / n, var = (P / n) (Q / n), which IS
//                     the law of total variance of a Bernoulli mixture and has no cancellation near 0 or 1.
//   linear, Poisson   sums of (mu - c) and (mu - c)^2 with c the row's first finite mu of that wave: the between-draw sum of squares
//                     S2 - S1^2 / k loses nothing to the size of mu, and is exactly 0 when every draw of the row is equal.
// The two wm waves that share a row block are combined once at the end, wm = 0 first, by the wm = 0 wave (Chan's pairwise form
// for the shifted sums; a wave that owned no draw has count 0 and is left out, never divided by): deterministic, no atomics, no
// n x rows intermediate.  One rounding to float32 from float64 per output.
// Non-finite values: a NaN t makes the row's mean and variance NaN.  An infinite mu is not added to the sums (inf - inf) but
// remembered: a row with a +inf mu gives (+inf, +inf) (linear, t = -inf: (-inf, +inf); both signs: NaN, as the mean is).
#include "d3p_device.h"
#include "d3p_glm_tile.h"
#include "d3p_host.h"
#include "d3p_shifted_sums.h"

namespace d3p {

struct MomentsArgs {
    const float* X;
    uint64_t rows;
    int d, w_off, b_col;
    const float* lat;
    int64_t ld;
    uint32_t n;
    float sigma;   // LINREG: the observation's standard deviation
    float* mean;
    float* var;
};

template <int FAMILY>
// Registers: as k_loglik's lppd form, one wave per SIMD (the staging addresses live across the draw-tile loop); no scratch.
__global__ void __launch_bounds__(256, 1) k_moments(MomentsArgs g)
{
    // [k][draw] | [k][row] during the product; afterwards the same bytes hold each wave's t, half a tile at a time (4 x 32 x 65 floats)
    __shared__ __attribute__((aligned(16))) float smem[D3P_TILE_SMEM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const uint64_t r0 = (uint64_t)blockIdx.x * D3P_TILE_N;
    const uint64_t r = r0 + wn * 64 + lane;   // lane l owns row r in the epilogue
    const bool live = r < g.rows;
    double a0 = 0.0, a1 = 0.0;   // LOGREG: sum p, sum q; else: sum (mu - c), sum (mu - c)^2
    float c = 0.f;               // the shift: this wave's first finite mu of the row
    uint32_t cnt = 0, inf_seen = 0;   // values in the sums; bit 0: a +inf mu came by, bit 1: a -inf one
    for (uint32_t s0 = 0; s0 < g.n; s0 += D3P_TILE_M) {
        tile_f16v acc[2][2];
        tile_product(smem, g, r0, s0, acc);
        float* L = tile_block(smem);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            tile_scatter(L, acc[mb][0], acc[mb][1]);
            __syncthreads();
            if (live) {
#pragma clang fp contract(off)
                for (int i = 0; i < 32; ++i) {
                    const uint32_t s = s0 + wm * 64 + mb * 32 + i;
                    if (s >= g.n) break;
                    float t = L[i * 65 + lane];
                    if (g.b_col >= 0) t = t + g.lat[(size_t)s * g.ld + g.b_col];
                    if (FAMILY == D3P_FAMILY_LOGREG) {
                        float p, q;
                        sigmoid_pair(t, p, q);   // p = sigmoid(t), q = sigmoid(-t)   (a NaN t: both NaN)
                        a0 += (double)p;
                        a1 += (double)q;
                    } else {
                        const float mu = glm_mean<FAMILY>(t);
                        if (fabsf(mu) == INFINITY) {
                            inf_seen |= mu > 0.0f ? 1u : 2u;
                        } else {
                            if (cnt == 0) c = mu;
                            const double dv = (double)mu - (double)c;
                            a0 += dv;
                            a1 += dv * dv;
                            ++cnt;
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    // the two waves of a row block: wm = 1 hands its sums over, wm = 0 merges (its own first) and finishes in float64
    double* S = reinterpret_cast<double*>(smem);   // [2][128] sums, then [128] shifts, counts and flags behind them
    float* Cs = smem + 4 * D3P_TILE_N;
    uint32_t* Ks = reinterpret_cast<uint32_t*>(smem + 5 * D3P_TILE_N);
    uint32_t* Fs = reinterpret_cast<uint32_t*>(smem + 6 * D3P_TILE_N);
    const int slot = wn * 64 + lane;
    if (wm == 1) { S[slot] = a0; S[D3P_TILE_N + slot] = a1; Cs[slot] = c; Ks[slot] = cnt; Fs[slot] = inf_seen; }
    __syncthreads();
    if (wm == 0 && live) {
        const double b0 = S[slot], b1 = S[D3P_TILE_N + slot];
        const double nd = (double)g.n;
        double mean, var;
        if (FAMILY == D3P_FAMILY_LOGREG) {
            mean = (a0 + b0) / nd;
            var = mean * ((a1 + b1) / nd);
        } else {
            const uint32_t ka = cnt, kb = Ks[slot];
            double ma = 0.0, qa = 0.0, mb = 0.0, qb = 0.0, m2;
            if (ka) moments_part(ka, c, a0, a1, ma, qa);
            if (kb) moments_part(kb, Cs[slot], b0, b1, mb, qb);
            if (!kb) { mean = ma; m2 = qa; }          // (neither: 0, 0 -- every mu was infinite, handled below)
            else if (!ka) { mean = mb; m2 = qb; }
            else {
                const double tot = (double)ka + (double)kb, delta = mb - ma;
                mean = ma + delta * ((double)kb / tot);
                m2 = (qa + qb) + (delta * delta) * ((double)ka * (double)kb / tot);
            }
            const double within = FAMILY == D3P_FAMILY_LINREG ? (double)g.sigma * (double)g.sigma : mean;
            var = within + m2 / nd;
            const uint32_t f = inf_seen | Fs[slot];
            if (f && !(mean != mean)) {               // a NaN t keeps the row NaN
                mean = f == 1u ? (double)INFINITY : f == 2u ? -(double)INFINITY : (double)NAN;
                var = f == 3u ? (double)NAN : (double)INFINITY;
            }
        }
        g.mean[r] = (float)mean;   // (a finite float64 beyond float32's range rounds to inf)
        g.var[r] = (float)var;
    }
}

}  // namespace d3p

using namespace d3p;

extern "C" {

int d3p_predict_moments(void* stream, const d3p_logreg_model* model, const float* X_dev, uint64_t rows, const float* latent_dev,
                        int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, float* mean_rows_dev, float* var_rows_dev)
{
    const char* what = "d3p_predict_moments";
    const d3p_logreg_model* m = model;
    // (there are no labels: validate_model's label check gets a pointer that is not null)
    if (int rc = validate_model(m, m, what)) return rc;   // D3P_GUIDE_EXP_SITES: D3P_E_UNSUPPORTED (the guide transform is not read otherwise)
    bool launch;
    if (int rc = glm_tile_check(what, m, rows, latent_ld, w_off, b_col, n, {X_dev, latent_dev, mean_rows_dev, var_rows_dev}, "X / latent / mean / var",
                                "X, latent, mean and var", &launch); rc || !launch)
        return rc;
    MomentsArgs g;
    g.X = X_dev; g.rows = rows; g.d = m->d; g.w_off = w_off; g.b_col = b_col; g.lat = latent_dev; g.ld = latent_ld; g.n = n;
    g.sigma = m->family == D3P_FAMILY_LINREG ? m->lik_sigma : 0.f;
    g.mean = mean_rows_dev; g.var = var_rows_dev;
    const dim3 grid(cdiv(rows, D3P_TILE_N));
    hipStream_t s = (hipStream_t)stream;
    if (m->family == D3P_FAMILY_LINREG) hipLaunchKernelGGL((k_moments<D3P_FAMILY_LINREG>), grid, dim3(256), 0, s, g);
    else if (m->family == D3P_FAMILY_POISSON) hipLaunchKernelGGL((k_moments<D3P_FAMILY_POISSON>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((k_moments<D3P_FAMILY_LOGREG>), grid, dim3(256), 0, s, g);
    return check_launch(what);
}

}  // extern "C"
