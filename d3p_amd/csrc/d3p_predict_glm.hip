// Predictive sampling of the linear and Poisson regression families (d3p_amd/predictive.py): the outcomes of the observed site over
// n latent draws, fused with the draws x rows product -- t, eps and the uniforms never reach memory.
//   t[s, r]   = X[r] . w_s (+ b_s)                                                      float32, from the tile
//   linear    obs[s, r] = fl(t + fl(eps sigma)), eps = normal(obs_key_s, (rows,))[r]    float32   (numpyro Normal.sample)
//   Poisson   obs[s, r] = poisson_draw(exp(t), the uniforms of obs_key_s)               int32     (the project's own rule, below)
//
// The product is the shared tile (d3p_glm_tile.h): 128 draws x 128 rows per workgroup, 4 wavefronts (2 x 2) of 64 x 64, the grid over
// (row tiles, draw tiles); the accumulators go through LDS so that lane l owns row l and walks 32 draws: a store is 64 consecutive
// words.
//
// The Poisson rule (UNPINNED and the project's own -- jax.random.poisson draws with whole-array while_loops
// whose text is not available to this build, so no bit parity with it is claimed; the position d3po_gamma_sample takes for
// jax.random.gamma).  lam = expf(t) in float32 as in k_loglik / k_moments; everything after it in float64 on L = (double) lam.
//   uniforms   (U_j, V_j) of iteration j >= 0 are elements [r] and [rows + r] of uniform(fold_in(obs_key_s, j), (2 rows,)): in jax's
//              layout the two words of ONE threefry call with the counter pair (r, rows + r).  Needs 2 rows < 2^32.
//   special    NaN t: -1;  lam == 0: 0;  lam == +inf or a draw above 2^31 - 1: 2147483647.
//   lam < 10   inversion on U_0: p = exp(-L), F = p, k = 0; while U_0 >= F and k < 64: k += 1, p *= L / k, F += p.
//   lam >= 10  Hoermann's transformed rejection (PTRS, 1993): s = sqrt(L), b = 0.931 + 2.53 s, a = -0.059 + 0.02483 b,
//              1/alpha = 1.1239 + 1.1328 / (b - 3.4), v_r = 0.9277 - 3.6224 / (b - 2).  Iteration j: u = U_j - 0.5, us = 0.5 - |u|,
//              k = floor((2 a / us + b) u + L + 0.43); accept if us >= 0.07 && V_j <= v_r; otherwise retry if k < 0 || (us < 0.013 &&
//              V_j > us); otherwise accept iff log V_j + log(1/alpha) - log(a / us^2 + b) <= -L + k log L - lgamma(k + 1).  At most
//              64 iterations, then floor(L).
// Every loop has a fixed cap.  fold_in(obs_key_s, j) is the same for every row of a draw: iteration 0's key, the only one every
// outcome needs, is derived once per draw and workgroup into LDS; a later iteration (0.13 to 0.33 per outcome) derives its own.
#include "d3p_device.h"
#include "d3p_glm_tile.h"
#include "d3p_host.h"
#include "d3p_outcome.h"

namespace d3p {

struct GlmPredictArgs {
    const float* X;
    uint64_t rows;
    int d, w_off, b_col;
    const float* lat;
    int64_t ld;
    uint32_t n;
    float sigma;   // LINREG: the observation's standard deviation
    const uint32_t* obs_keys;
    void* obs;     // LINREG: float32, POISSON: int32; n x rows
};

// (glm_uniform_pair and poisson_draw, the rule of the comment above: d3p_outcome.h, shared with k_predict_stats)

template <int FAMILY>
__global__ void __launch_bounds__(256) k_predict_glm(GlmPredictArgs g)
{
    // [k][draw] | [k][row] during the product; afterwards the same bytes hold each wave's t, half a tile at a time
    __shared__ float smem[D3P_TILE_SMEM];
    __shared__ uint32_t keys[D3P_TILE_M][4];   // per draw of the tile: the obs key and fold_in(obs key, 0)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const uint64_t r0 = (uint64_t)blockIdx.x * D3P_TILE_N;
    const uint32_t s0 = blockIdx.y * D3P_TILE_M;
    stage_obs_keys<FAMILY>(keys, g.obs_keys, s0, g.n);
    tile_f16v acc[2][2];
    tile_product(smem, g, r0, s0, acc);
    // Epilogue, per half of the wave's 64 draws: the accumulators go to LDS ([draw 0..31][row 0..63], rows padded to 65 floats), then
    // lane l owns row l and walks the 32 draws; the accumulators are dead from there on, so the outcome rule has the registers
    float* L = tile_block(smem);
    const uint64_t r = r0 + wn * 64 + lane;
#pragma unroll 1
    for (int mb = 0; mb < 2; ++mb) {
        tile_scatter(L, mb == 0 ? acc[0][0] : acc[1][0], mb == 0 ? acc[0][1] : acc[1][1]);   // (selected by hand: the loop is not unrolled)
        __syncthreads();
        if (r < g.rows) {
#pragma unroll 1
            for (int i = 0; i < 32; ++i) {
                const int sl = wm * 64 + mb * 32 + i;
                const uint32_t s = s0 + sl;
                if (s >= g.n) break;
                float t = L[i * 65 + lane];
                if (g.b_col >= 0) t = t + g.lat[(size_t)s * g.ld + g.b_col];
                const size_t at = (size_t)s * g.rows + r;
                if (FAMILY == D3P_FAMILY_LINREG) {
                    const float eps = bits_to_normal(tf_iota_word(keys[sl][0], keys[sl][1], g.rows, r));
                    static_cast<float*>(g.obs)[at] = normal_site_value(t, eps, g.sigma);
                } else {
                    static_cast<int32_t*>(g.obs)[at] = poisson_draw(t, keys[sl][0], keys[sl][1], keys[sl][2], keys[sl][3], (uint32_t)g.rows, (uint32_t)r);
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace d3p

using namespace d3p;

extern "C" {

int d3p_predict_glm(void* stream, const d3p_logreg_model* model, const float* X_dev, uint64_t rows, int32_t d, const float* latent_dev,
                    int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, const uint32_t* obs_keys_dev, void* obs_dev)
{
    const char* what = "d3p_predict_glm";
    const d3p_logreg_model* m = model;
    // (there are no labels: validate_model's label check gets a pointer that is not null)
    if (int rc = validate_model(m, m, what)) return rc;   // D3P_GUIDE_EXP_SITES: D3P_E_UNSUPPORTED; LINREG: lik_sigma finite and > 0
    if (!is_glm(m))
        return fail(D3P_E_UNSUPPORTED, "%s: linear and Poisson regression only (logistic regression: d3p_predict_logreg; the Gaussian mean: "
                    "d3p_predict_gauss)", what);
    if (d != m->d) return fail(D3P_E_INVALID_ARG, "%s: d = %d differs from the model's %d", what, d, m->d);
    if (m->family == D3P_FAMILY_POISSON && 2 * rows > 0xFFFFFFFFull)
        return fail(D3P_E_INVALID_ARG, "%s: Poisson outcomes need 2 rows < 2^32 (one threefry stream of 2 rows uniforms per iteration)", what);
    bool launch;
    if (int rc = glm_tile_check(what, m, rows, latent_ld, w_off, b_col, n, {X_dev, latent_dev, obs_keys_dev, obs_dev}, "X / latent / obs_keys / obs",
                                "X, latent, obs_keys and obs", &launch); rc || !launch)
        return rc;
    GlmPredictArgs g;
    g.X = X_dev; g.rows = rows; g.d = d; g.w_off = w_off; g.b_col = b_col; g.lat = latent_dev; g.ld = latent_ld; g.n = n;
    g.sigma = m->family == D3P_FAMILY_LINREG ? m->lik_sigma : 0.f;
    g.obs_keys = obs_keys_dev; g.obs = obs_dev;
    const dim3 grid(cdiv(rows, D3P_TILE_N), cdiv(n, D3P_TILE_M));
    hipStream_t s = (hipStream_t)stream;
    if (m->family == D3P_FAMILY_LINREG) hipLaunchKernelGGL((k_predict_glm<D3P_FAMILY_LINREG>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((k_predict_glm<D3P_FAMILY_POISSON>), grid, dim3(256), 0, s, g);
    return check_launch(what);
}

}  // extern "C"
