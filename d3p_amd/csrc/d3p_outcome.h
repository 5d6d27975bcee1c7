// The outcome rules of the regression families' observed site, one definition each, shared by the kernels that STORE the outcomes
//   k_predict_logreg (d3p_predict.hip)   k_predict_vae_obs (d3p_predict.hip)   k_predict_glm (d3p_predict_glm.hip)
// and the kernels that REDUCE them per draw without storing them
//   k_predict_stats (d3p_rep_stats.hip)   k_predict_discrepancy (d3p_discrepancy.hip)
// The linear family's rule, normal_site_value, lives beside the tile (d3p_glm_tile.h).  Which numpyro / jax function each restates:
// the file comments of d3p_predict.hip and d3p_predict_glm.hip, DESIGN.md section 4b.
// glm_outcome<FAMILY> is the choice among the three rules per element, stage_obs_keys<FAMILY> the per-draw keys they take.
#pragma once
#include "d3p_device.h"
#include "d3p_glm_tile.h"

namespace d3p {

// BernoulliLogits.probs = expit(logits) = 1 / (1 + exp(-logits))
__device__ __forceinline__ float sigmoid_probs(float logit) { return 1.0f / (1.0f + expf(-logit)); }

// numpyro Bernoulli.sample = jax.random.bernoulli(key, probs, shape) = uniform(key, shape) < probs, returned as int32; `bits` is
// word j of the site's threefry stream (jax's array layout: flat index j = row * width + col)
__device__ __forceinline__ int32_t bernoulli_draw(uint32_t bits, float p) { return bits_to_uniform(bits, 0.0f, 1.0f) < p ? 1 : 0; }

// (U, V) = elements [r] and [rows + r] of jax.random.uniform(key, (2 rows,)): one threefry call, counter pair (r, rows + r)
__device__ __forceinline__ void glm_uniform_pair(uint32_t k0, uint32_t k1, uint32_t rows, uint32_t r, double& U, double& V)
{
    uint32_t a, b;
    threefry2x32(k0, k1, r, rows + r, a, b);
    U = (double)bits_to_uniform(a, 0.0f, 1.0f);
    V = (double)bits_to_uniform(b, 0.0f, 1.0f);
}

// The Poisson rule of d3p_predict_glm.hip's file comment.  (o0, o1): the draw's obs key; (f0, f1) = fold_in of it with 0.
__device__ __forceinline__ int32_t poisson_draw(float t, uint32_t o0, uint32_t o1, uint32_t f0, uint32_t f1, uint32_t rows, uint32_t r)
{
#pragma clang fp contract(off)
    if (t != t) return -1;
    const float lam = expf(t);
    if (lam == 0.0f) return 0;
    if (lam == INFINITY) return 2147483647;
    const double L = (double)lam;
    double U, V, k;
    glm_uniform_pair(f0, f1, rows, r, U, V);
    if (lam < 10.0f) {
        double p = exp(-L), F = p;
        k = 0.0;
        while (U >= F && k < 64.0) {
            k += 1.0;
            p *= L / k;
            F += p;
        }
    } else {
        const double s = sqrt(L);
        const double b = 0.931 + 2.53 * s;
        const double a = -0.059 + 0.02483 * b;
        const double log_inv_alpha = log(1.1239 + 1.1328 / (b - 3.4));
        const double vr = 0.9277 - 3.6224 / (b - 2.0);
        const double logL = log(L);
        k = floor(L);   // what 64 rejections leave
        for (uint32_t j = 0; j < 64u; ++j) {
            if (j > 0u) {
                uint32_t g0, g1;
                threefry2x32(o0, o1, 0u, j, g0, g1);   // jax.random.fold_in(obs_key, j)
                glm_uniform_pair(g0, g1, rows, r, U, V);
            }
            const double u = U - 0.5;
            const double us = 0.5 - fabs(u);
            const double kk = floor((2.0 * a / us + b) * u + L + 0.43);
            if (us >= 0.07 && V <= vr) { k = kk; break; }
            if (kk < 0.0 || (us < 0.013 && V > us)) continue;
            if (log(V) + log_inv_alpha - log(a / (us * us) + b) <= -L + kk * logL - lgamma(kk + 1.0)) { k = kk; break; }
        }
    }
    return k > 2147483647.0 ? 2147483647 : (int32_t)k;
}

// keys[draw of the tile] = the draw's obs key and, for Poisson, fold_in(obs key, 0) (zeros past n), once per workgroup.  Called by
// every thread before the first tile_product, which runs at least once (d >= 1, a strip has a tile): the product's barriers come
// between this and the readers.
template <int FAMILY>
__device__ __forceinline__ void stage_obs_keys(uint32_t (*keys)[4], const uint32_t* obs_keys, uint32_t s0, uint32_t n)
{
    const int tid = threadIdx.x;
    if (tid < D3P_TILE_M) {
        const uint32_t s = s0 + tid;
        uint32_t o0 = 0u, o1 = 0u, f0 = 0u, f1 = 0u;
        if (s < n) {
            o0 = obs_keys[2 * (size_t)s];
            o1 = obs_keys[2 * (size_t)s + 1];
            if (FAMILY == D3P_FAMILY_POISSON) threefry2x32(o0, o1, 0u, 0u, f0, f1);   // jax.random.fold_in(obs_key, 0)
        }
        keys[tid][0] = o0; keys[tid][1] = o1; keys[tid][2] = f0; keys[tid][3] = f1;
    }
}

// The outcome of row r of `rows` at the predictor t under the draw's staged key words (o0, o1, f0, f1): float32 for the linear
// family (sigma: the observation's standard deviation), int32 for Poisson and logistic -- what k_predict_glm / k_predict_logreg store
template <int FAMILY>
__device__ __forceinline__ auto glm_outcome(float t, uint32_t o0, uint32_t o1, uint32_t f0, uint32_t f1, uint64_t rows, uint64_t r, float sigma)
{
    if constexpr (FAMILY == D3P_FAMILY_LINREG) return normal_site_value(t, bits_to_normal(tf_iota_word(o0, o1, rows, r)), sigma);
    else if constexpr (FAMILY == D3P_FAMILY_POISSON) return poisson_draw(t, o0, o1, f0, f1, (uint32_t)rows, (uint32_t)r);
    else return bernoulli_draw(tf_iota_word(o0, o1, rows, r), sigmoid_probs(t));
}

}  // namespace d3p
