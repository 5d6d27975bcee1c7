// Predictive sampling of the linear and Poisson regression families (d3p_amd/predictive.py): the outcomes of the observed site over
// n latent draws, fused with the draws x rows product -- t, eps and the uniforms never reach memory.
//   t[s, r]   = X[r] . w_s (+ b_s)                                                      float32, from the tile
//   linear    obs[s, r] = fl(t + fl(eps sigma)), eps = normal(obs_key_s, (rows,))[r]    float32   (numpyro Normal.sample)
//   Poisson   obs[s, r] = poisson_draw(exp(t), the uniforms of obs_key_s)               int32     (the project's own rule, below)
//
// The product is k_predict_logreg's tile (d3p_predict.hip): 128 draws x 128 rows per workgroup, 4 wavefronts (2 x 2) of 64 x 64, K in
// slices of 32 staged through LDS, v_mfma_f32_32x32x2_f32 (exact float32 products), the grid over (row tiles, draw tiles); the
// accumulators go through LDS so that lane l owns row l and walks 32 draws: a store is 64 consecutive words.  It is a FOURTH COPY of
// that loop, on purpose, as the third was (d3p_moments.hip): sharing it changed k_predict_logreg's generated code (DESIGN.md sections
// 4c, 4d, 4e); unifying the four is a refactor of its own with its own measurements.
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
#include "d3p_host.h"

namespace d3p {

#define D3P_PG_TM 128
#define D3P_PG_TN 128
#define D3P_PG_TK 32
#define D3P_PG_LD (D3P_PG_TN + 4)
typedef float predict_glm_f16v __attribute__((ext_vector_type(16)));

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

// numpyro Normal.sample: loc + random.normal(key, shape) * scale -- a product, then a sum (two roundings); normal_site_value's rule
// (d3p_predict.hip), restated here because that file's text is pinned.  The pragma keeps hipcc from contracting them into one fma.
__device__ __forceinline__ float glm_normal_value(float loc, float eps, float scale)
{
#pragma clang fp contract(off)
    return loc + eps * scale;
}

// (U, V) = elements [r] and [rows + r] of jax.random.uniform(key, (2 rows,)): one threefry call, counter pair (r, rows + r)
__device__ __forceinline__ void glm_uniform_pair(uint32_t k0, uint32_t k1, uint32_t rows, uint32_t r, double& U, double& V)
{
    uint32_t a, b;
    threefry2x32(k0, k1, r, rows + r, a, b);
    U = (double)bits_to_uniform(a, 0.0f, 1.0f);
    V = (double)bits_to_uniform(b, 0.0f, 1.0f);
}

// The Poisson rule of the file comment.  (o0, o1): the draw's obs key; (f0, f1) = fold_in of it with 0.
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

template <int FAMILY>
__global__ void __launch_bounds__(256) k_predict_glm(GlmPredictArgs g)
{
    // [k][draw] | [k][row] during the product; afterwards the same bytes hold each wave's t, half a tile at a time
    __shared__ float smem[2 * D3P_PG_TK * D3P_PG_LD];
    __shared__ uint32_t keys[D3P_PG_TM][4];   // per draw of the tile: the obs key and fold_in(obs key, 0)
    float (*As)[D3P_PG_LD] = reinterpret_cast<float (*)[D3P_PG_LD]>(smem);
    float (*Bs)[D3P_PG_LD] = reinterpret_cast<float (*)[D3P_PG_LD]>(smem + D3P_PG_TK * D3P_PG_LD);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const uint64_t r0 = (uint64_t)blockIdx.x * D3P_PG_TN;
    const uint32_t s0 = blockIdx.y * D3P_PG_TM;
    const int d = g.d;
    if (tid < D3P_PG_TM) {   // (read after the barriers of the product loop, which runs at least once: d >= 1)
        const uint32_t s = s0 + tid;
        uint32_t o0 = 0u, o1 = 0u, f0 = 0u, f1 = 0u;
        if (s < g.n) {
            o0 = g.obs_keys[2 * (size_t)s];
            o1 = g.obs_keys[2 * (size_t)s + 1];
            if (FAMILY == D3P_FAMILY_POISSON) threefry2x32(o0, o1, 0u, 0u, f0, f1);   // jax.random.fold_in(obs_key, 0)
        }
        keys[tid][0] = o0; keys[tid][1] = o1; keys[tid][2] = f0; keys[tid][3] = f1;
    }
    predict_glm_f16v acc[2][2];
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
    for (int kc = 0; kc < d; kc += D3P_PG_TK) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = tid + 256 * q;
            As[e & 31][e >> 5] = ra[q];
            Bs[e & 31][e >> 5] = rb[q];
        }
        __syncthreads();
        if (kc + D3P_PG_TK < d) fetch(kc + D3P_PG_TK);   // next slice in flight while this one multiplies
#pragma unroll
        for (int kk = 0; kk < D3P_PG_TK; kk += 2) {
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
    // Epilogue, per half of the wave's 64 draws: the accumulators go to LDS ([draw 0..31][row 0..63], rows padded to 65 floats), then
    // lane l owns row l and walks the 32 draws; the accumulators are dead from there on, so the outcome rule has the registers
    float* L = smem + wave * (32 * 65);
    const uint64_t r = r0 + wn * 64 + lane;
#pragma unroll 1
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float av = mb == 0 ? acc[0][nb][v] : acc[1][nb][v];
                L[(8 * (v >> 2) + 4 * (lane >> 5) + (v & 3)) * 65 + nb * 32 + (lane & 31)] = av;
            }
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
                    static_cast<float*>(g.obs)[at] = glm_normal_value(t, eps, g.sigma);
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
    if (!X_dev || !latent_dev || !obs_keys_dev || !obs_dev) return fail(D3P_E_INVALID_ARG, "%s: null X / latent / obs_keys / obs pointer", what);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n must be >= 1", what);
    if (!(w_off >= 0 && (int64_t)w_off + d <= latent_ld && b_col < latent_ld && b_col >= -1 && !(b_col >= w_off && b_col < w_off + d)))
        return fail(D3P_E_INVALID_ARG, "%s: the weights [w_off, w_off + d) and the intercept column must lie in a latent row, apart", what);
    if ((m->intercept != 0) != (b_col >= 0)) return fail(D3P_E_INVALID_ARG, "%s: b_col must be given exactly when the model has an intercept", what);
    if (rows > 0xFFFFFFFFull || cdiv(rows, D3P_PG_TN) > 0x7fffffffu || cdiv(n, D3P_PG_TM) > 65535u)
        return fail(D3P_E_INVALID_ARG, "%s: rows <= 2^32 - 1 and n <= 128 x 65535", what);
    if (m->family == D3P_FAMILY_POISSON && 2 * rows > 0xFFFFFFFFull)
        return fail(D3P_E_INVALID_ARG, "%s: Poisson outcomes need 2 rows < 2^32 (one threefry stream of 2 rows uniforms per iteration)", what);
    if (rows == 0) return D3P_OK;
    if (!is_device_ptr(X_dev) || !is_device_ptr(latent_dev) || !is_device_ptr(obs_keys_dev) || !is_device_ptr(obs_dev))
        return fail(D3P_E_INVALID_ARG, "%s: X, latent, obs_keys and obs must be device memory", what);
    GlmPredictArgs g;
    g.X = X_dev; g.rows = rows; g.d = d; g.w_off = w_off; g.b_col = b_col; g.lat = latent_dev; g.ld = latent_ld; g.n = n;
    g.sigma = m->family == D3P_FAMILY_LINREG ? m->lik_sigma : 0.f;
    g.obs_keys = obs_keys_dev; g.obs = obs_dev;
    const dim3 grid(cdiv(rows, D3P_PG_TN), cdiv(n, D3P_PG_TM));
    hipStream_t s = (hipStream_t)stream;
    if (m->family == D3P_FAMILY_LINREG) hipLaunchKernelGGL((k_predict_glm<D3P_FAMILY_LINREG>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((k_predict_glm<D3P_FAMILY_POISSON>), grid, dim3(256), 0, s, g);
    return check_launch(what);
}

}  // extern "C"
