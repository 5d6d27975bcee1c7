// The draws x rows product tile of the regression kernels: t[s, r] = X[r] . w_s on a workgroup tile of 128 draws x 128 rows, used by
//   k_predict_logreg (d3p_predict.hip)   k_loglik (d3p_loglik.hip)   k_moments (d3p_moments.hip)   k_predict_glm (d3p_predict_glm.hip)
//   k_draw_sums (d3p_draw_sums.hip)   k_mean_rows (d3p_quantiles.hip)   k_predict_stats (d3p_rep_stats.hip)
//   k_predict_discrepancy (d3p_discrepancy.hip)
// which differ only in what they do with t.  One copy of the staging, the matrix-core loop and the accumulator scatter, and one
// copy of the argument checks their C entries share (measurements: docs/experiments_glm_tile.md).
//
// Workgroup: 256 threads = 4 wavefronts (2 x 2: wm = draw half, wn = row half) of 64 x 64, K in slices of 32 staged through LDS (X
// and the draws' weights, both transposed to [k][.] so that a fragment read is 32 consecutive floats).  Product on the matrix cores:
// v_mfma_f32_32x32x2_f32, exact float32 products, lane l: A row / B column l % 32, k = l / 32; D[i][j] with j = l % 32,
// i = 8 (v / 4) + 4 (l / 32) + v % 4.  A = the draws' weights (i = draw), B = X^T (j = row): the 32 lanes of a half-wave hold 32
// consecutive rows.  X is read once per tile of 128 draws; the weights of a tile (128 x d) are re-read per row tile from L2 in K
// slices (at d = 512 they would be 256 KB of LDS).
#pragma once
#include "d3p_device.h"
#include "d3p_host.h"

#include <initializer_list>

namespace d3p {

#define D3P_TILE_M 128                   // draws
#define D3P_TILE_N 128                   // rows
#define D3P_TILE_K 32
#define D3P_TILE_LD (D3P_TILE_N + 4)     // padded leading dimension of a staged slice
#define D3P_TILE_SMEM (2 * D3P_TILE_K * D3P_TILE_LD)   // floats: [k][draw] | [k][row]; afterwards 4 waves x [32][65]
typedef float tile_f16v __attribute__((ext_vector_type(16)));

// numpyro Normal.sample: loc + random.normal(key, shape) * scale -- a product, then a sum (two roundings, no fused multiply-add).
// The pragma is what keeps them apart: hipcc contracts across inlined code by default, and HIP's __fadd_rn / __fmul_rn are plain
// `+` / `*` there, so without it the product and the sum became one v_fma_f32 (tests/test_gpu_predictive_edges.py checks the two
// roundings bit for bit)
__device__ __forceinline__ float normal_site_value(float loc, float eps, float scale)
{
#pragma clang fp contract(off)
    return loc + eps * scale;
}

// acc[a][b] = the wave's 32 x 32 block (draw half a, row half b) of the tile at rows r0.., draws s0..; smem: D3P_TILE_SMEM floats.
// Args: X, rows, d, lat, ld, w_off, n.  Rows and draws beyond the end and k >= d are staged as zeros.  Ends on a barrier: smem is free.
template <class Args>
__device__ __forceinline__ void tile_product(float* smem, const Args& g, uint64_t r0, uint32_t s0, tile_f16v (&acc)[2][2])
{
    float (*As)[D3P_TILE_LD] = reinterpret_cast<float (*)[D3P_TILE_LD]>(smem);
    float (*Bs)[D3P_TILE_LD] = reinterpret_cast<float (*)[D3P_TILE_LD]>(smem + D3P_TILE_K * D3P_TILE_LD);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int d = g.d;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[a][b][v] = 0.f;
    // staging: element e = tid + 256 q of a slice -> (tile row e / 32, k e % 32): 32 consecutive threads read 128 contiguous bytes
    float ra[16], rb[16];
    auto fetch = [&](int kc) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = tid + 256 * q, row = e >> 5, k = kc + (e & 31);
            const uint32_t s = s0 + row;
            const uint64_t r = r0 + row;
            ra[q] = (s < g.n && k < d) ? g.lat[(size_t)s * g.ld + g.w_off + k] : 0.f;
            rb[q] = (r < g.rows && k < d) ? g.X[r * (uint64_t)d + k] : 0.f;
        }
    };
    fetch(0);
    for (int kc = 0; kc < d; kc += D3P_TILE_K) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = tid + 256 * q;
            As[e & 31][e >> 5] = ra[q];
            Bs[e & 31][e >> 5] = rb[q];
        }
        __syncthreads();
        if (kc + D3P_TILE_K < d) fetch(kc + D3P_TILE_K);   // next slice in flight while this one multiplies
#pragma unroll
        for (int kk = 0; kk < D3P_TILE_K; kk += 2) {
            const int k = kk + (lane >> 5), c = lane & 31;
            const float a0 = As[k][wm * 64 + c], a1 = As[k][wm * 64 + 32 + c];
            const float b0 = Bs[k][wn * 64 + c], b1 = Bs[k][wn * 64 + 32 + c];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
}

// One draw half of a wave's accumulators (h0 | h1 = its row halves) into the wave's LDS block L = tile_block(smem):
// [draw 0..31][row 0..63], rows padded to 65 floats, so that afterwards lane l owns row l and walks the 32 draws at L[i * 65 + l].
// The caller puts a barrier after it, and one before the next half overwrites the block.
__device__ __forceinline__ float* tile_block(float* smem) { return smem + (threadIdx.x >> 6) * (32 * 65); }

__device__ __forceinline__ void tile_scatter(float* L, const tile_f16v& h0, const tile_f16v& h1)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        float* p = L + (8 * (v >> 2) + 4 * (lane >> 5) + (v & 3)) * 65 + (lane & 31);
        p[0] = h0[v];
        p[32] = h1[v];
    }
}

// ---- the pointwise log-likelihood of the forms that reduce it: k_loglik (d3p_loglik.hip) and k_draw_sums (d3p_draw_sums.hip) ---------
// log p(y | t): the `ll` of glm_link (d3p_logreg_kernel.h) without its gradient half, same expressions and rounding order for the
// linear and the Poisson family; c = glm_label_const's value (LINREG: ll_const, POISSON: lgammaf(y + 1)), once per row.  No clamps:
// exp(t) = inf gives -inf, what float32 jax computes.
// LOGREG differs from glm_link's y t - softplus(t) ON PURPOSE: that form cancels where the label is predicted well (y = 1, t = 4:
// 4 - 4.018, half an ulp of 4 against a result of 0.018), which a loss summed over a batch never sees and a per-element bound does.
// Here ll = -(max(t, 0) - y t + log1p(exp(-|t|))) with max(t, 0) - y t taken as (1 - y) t (t >= 0) or -y t (t < 0): exact for
// y in {0, 1} (-softplus(-t) resp. -softplus(t)), and numpyro's BernoulliLogits.log_prob for any y in [0, 1].
template <int FAMILY>
__device__ __forceinline__ float loglik_value(float t, float y, float nh, float c)
{
#pragma clang fp contract(off)
    if (FAMILY == D3P_FAMILY_LINREG) {
        const float r = t - y;
        return (nh * r) * r - c;
    }
    if (FAMILY == D3P_FAMILY_POISSON) {
        const float mu = expf(t);
        return (y * t - mu) - c;
    }
    const float lin = t >= 0.0f ? (1.0f - y) * t : -(y * t);
    return -(lin + log1pf(expf(-fabsf(t))));
}

// ---- the conditional mean E[y | t] of the forms that take it: k_moments (d3p_moments.hip), k_mean_rows (d3p_quantiles.hip) and
// k_predict_discrepancy (d3p_discrepancy.hip), whose float32 mu are bit for bit the same (tests/test_gpu_glm_tile.py) ----------------
// p = sigmoid(t) and q = sigmoid(-t) from ONE e = exp(-|t|): the larger is 1 / (1 + e), the smaller e / (1 + e); neither is 1 - the
// other.  A NaN t gives both NaN.  (No a * b + c shape: the including file's fp contract setting cannot change a bit.)
__device__ __forceinline__ void sigmoid_pair(float t, float& p, float& q)
{
    const float e = expf(-fabsf(t));
    const float den = 1.0f + e;
    const float big = 1.0f / den, small = e / den;
    p = t >= 0.0f ? big : small;
    q = t >= 0.0f ? small : big;
}

// mu = sigmoid(t) | t | exp(t)   (logistic | linear | Poisson); no clamps: exp(t) = inf stays inf
template <int FAMILY>
__device__ __forceinline__ float glm_mean(float t)
{
    if (FAMILY == D3P_FAMILY_LOGREG) {
        float p, q;
        sigmoid_pair(t, p, q);
        return p;
    }
    return FAMILY == D3P_FAMILY_POISSON ? expf(t) : t;
}

// ---- host: the argument checks of the C entries that take a model and a latent buffer (d3p_loglik_rows / _lppd, d3p_predict_moments,
// d3p_predict_glm), in the order those entries have always made them.  ptrs: X, the latent buffer and the entry's other buffers;
// null_names / dev_names: how the entry's two messages list them.  *launch = false with D3P_OK: rows == 0, nothing to do. -------------
inline int glm_tile_check(const char* what, const d3p_logreg_model* m, uint64_t rows, int64_t ld, int32_t w_off, int32_t b_col, uint32_t n,
                          std::initializer_list<const void*> ptrs, const char* null_names, const char* dev_names, bool* launch)
{
    *launch = false;
    if (m->family == D3P_FAMILY_GAUSS_MEAN)
        return fail(D3P_E_UNSUPPORTED, "%s: the Gaussian-mean family has no per-row linear predictor (logistic, linear and Poisson regression only)", what);
    for (const void* p : ptrs)
        if (!p) return fail(D3P_E_INVALID_ARG, "%s: null %s pointer", what, null_names);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n must be >= 1", what);
    const int d = m->d;
    if (!(w_off >= 0 && (int64_t)w_off + d <= ld && b_col < ld && b_col >= -1 && !(b_col >= w_off && b_col < w_off + d)))
        return fail(D3P_E_INVALID_ARG, "%s: the weights [w_off, w_off + d) and the intercept column must lie in a latent row, apart", what);
    if ((m->intercept != 0) != (b_col >= 0)) return fail(D3P_E_INVALID_ARG, "%s: b_col must be given exactly when the model has an intercept", what);
    if (rows > 0xFFFFFFFFull || cdiv(rows, D3P_TILE_N) > 0x7fffffffu || cdiv(n, D3P_TILE_M) > 65535u)
        return fail(D3P_E_INVALID_ARG, "%s: rows <= 2^32 - 1 and n <= 128 x 65535", what);
    if (rows == 0) return D3P_OK;
    for (const void* p : ptrs)
        if (!is_device_ptr(p)) return fail(D3P_E_INVALID_ARG, "%s: %s must be device memory", what, dev_names);
    *launch = true;
    return D3P_OK;
}

}  // namespace d3p
