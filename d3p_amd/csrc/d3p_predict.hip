// Prior and posterior predictive sampling (d3p/modelling.py:39-223): the draws of the latent sites, the fused
// logistic-regression predictive (n x rows product + Bernoulli draw, nothing but the int32 outcomes reaches HBM), the
// Gaussian-mean observations and the VAE's decoder pass over n draws.
//
// numpyro / jax are not importable in this build, so every sampling rule below is a RESTATEMENT (UNPINNED, DESIGN.md
// section 4b).  Each lives in exactly one device function, named in the comment with the numpyro / jax function it restates:
//   draw_key            modelling._sample_a_lot: keys = jax.random.split(rng_key, n), draw i = single-draw function of keys[i]
//   draw_chains         modelling.sample_posterior_predictive: model_key, guide_key = jax.random.split(key)
//   seed_site_key       numpyro.handlers.seed: `rng, site_key = split(rng)` at every sample statement that takes a key
//   normal_site_value   numpyro.distributions.Normal.sample: loc + random.normal(key, shape) * scale   (d3p_glm_tile.h: shared with d3p_predict_glm.hip)
//   bernoulli_draw      numpyro.distributions.Bernoulli(Logits / Probs).sample: random.uniform(key, shape) < probs
//   sigmoid_probs       BernoulliLogits.probs = jax.scipy.special.expit(logits)
// Which sites take a key (substituted / observed sites and a plate whose size equals its subsample size take none) is decided on
// the host (d3p_amd/modelling.py: site_plan) and arrives here as key indices.
#include "d3p_device.h"
#include "d3p_glm_tile.h"
#include "d3p_host.h"
#include "d3p_outcome.h"

namespace d3p {

// ---- the restated rules (one function each) ----------------------------------------------------------------------------------

// jax.random.split(key) (two children): words 0..3 of threefry_2x32(key, iota(4)) -> child 0 = (w0, w1), child 1 = (w2, w3)
__device__ __forceinline__ void split2(uint32_t k0, uint32_t k1, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1)
{
    threefry2x32(k0, k1, 0u, 2u, a0, b0);
    threefry2x32(k0, k1, 1u, 3u, a1, b1);
}

// modelling._sample_a_lot (modelling.py:134-136): draw i of the multi form runs on split(rng_key, n)[i]; the single form on rng_key
__device__ __forceinline__ void draw_key(const uint32_t* __restrict__ key, uint32_t n, int multi, uint32_t i, uint32_t& d0, uint32_t& d1)
{
    const uint32_t k0 = key[0], k1 = key[1];
    if (!multi) { d0 = k0; d1 = k1; return; }
    d0 = tf_iota_word(k0, k1, 2ull * n, 2ull * i);
    d1 = tf_iota_word(k0, k1, 2ull * n, 2ull * i + 1);
}

// modelling.sample_posterior_predictive (modelling.py:112): model_rng_key, guide_rng_key = split(rng_key); the prior
// predictive seeds the model with the draw's key itself (modelling.py:76)
__device__ __forceinline__ void draw_chains(uint32_t d0, uint32_t d1, int posterior, uint32_t (&model)[2], uint32_t (&guide)[2])
{
    if (!posterior) { model[0] = d0; model[1] = d1; guide[0] = guide[1] = 0u; return; }
    split2(d0, d1, model[0], model[1], guide[0], guide[1]);
}

// numpyro.handlers.seed: every sample statement that takes a key advances `rng, site_key = split(rng)`; `index` = how many
// such statements came before this one under the same handler
__device__ __forceinline__ void seed_site_key(const uint32_t (&chain)[2], int index, uint32_t& s0, uint32_t& s1)
{
    uint32_t c0 = chain[0], c1 = chain[1];
    for (int j = 0; j <= index; ++j) {
        uint32_t n0, n1;
        split2(c0, c1, n0, n1, s0, s1);
        c0 = n0; c1 = n1;
    }
}

// (sigmoid_probs and bernoulli_draw: d3p_outcome.h, shared with k_predict_stats)

// ---- latent draws ------------------------------------------------------------------------------------------------------------
#define D3P_PREDICT_MAX_SITES 8
struct DrawsArgs {
    const uint32_t* key;
    uint32_t n;
    int multi, posterior, n_sites, obs_chain, obs_index;
    d3p_predict_site site[D3P_PREDICT_MAX_SITES];
    float* latent;
    int64_t ld;
    uint32_t* obs_keys;
};

// grid (n, y): draw i = blockIdx.x; the y blocks stride over the word pairs of every site.  Every thread derives the keys itself
// (a few threefry calls: cheaper than a barrier and a broadcast).
__global__ void __launch_bounds__(256) k_predict_draws(DrawsArgs a)
{
    const uint32_t i = blockIdx.x;
    uint32_t d0, d1, chains[2][2];
    draw_key(a.key, a.n, a.multi, i, d0, d1);
    draw_chains(d0, d1, a.posterior, chains[0], chains[1]);
    if (a.obs_keys && a.obs_index >= 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        uint32_t s0, s1;
        seed_site_key(chains[a.obs_chain], a.obs_index, s0, s1);
        a.obs_keys[2 * (size_t)i] = s0;
        a.obs_keys[2 * (size_t)i + 1] = s1;
    }
    float* row = a.latent + (size_t)i * a.ld;
    const uint32_t stride = gridDim.y * blockDim.x, t0 = blockIdx.y * blockDim.x + threadIdx.x;
    for (int s = 0; s < a.n_sites; ++s) {
        const d3p_predict_site& st = a.site[s];
        float* out = row + st.offset;
        const uint32_t size = (uint32_t)st.size;
        if (st.key_index < 0) {   // substituted: the given value, the same for every draw
            for (uint32_t j = t0; j < size; j += stride) out[j] = st.value_dev[j];
            continue;
        }
        uint32_t k0, k1;
        seed_site_key(chains[st.chain], st.key_index, k0, k1);
        const uint32_t half = (size + 1) >> 1;
        for (uint32_t j = t0; j < half; j += stride) {
            const uint32_t j2 = j + half;
            uint32_t wa, wb;
            threefry2x32(k0, k1, j, j2 < size ? j2 : 0u, wa, wb);
            for (int h = 0; h < 2; ++h) {
                const uint32_t e = h ? j2 : j;
                if (e >= size) break;
                const float loc = st.loc_dev ? st.loc_dev[e] : st.loc_c;
                float sc = st.scale_c;
                if (st.scale_dev) sc = st.scale_kind == D3P_PREDICT_SCALE_EXP ? expf(st.scale_dev[e]) : st.scale_dev[e];
                out[e] = normal_site_value(loc, bits_to_normal(h ? wb : wa), sc);
            }
        }
    }
}

// ---- logistic regression: obs[s, r] = bernoulli(uniform(obs_key_s, rows)[r] < sigmoid(X[r] . w_s + b_s)) ----------------------
// The product is the shared tile (d3p_glm_tile.h): 128 draws x 128 rows per workgroup, 4 wavefronts (2 x 2) of 64 x 64; lane l of a
// half-wave holds row l, so the int32 outcomes leave in 128-byte segments.  The uniforms come from tf_iota_word (one threefry call
// per outcome, its second word discarded) in the epilogue.
struct LogregPredictArgs {
    const float* X;
    uint64_t rows;
    int d, w_off, b_col;
    const float* lat;
    int64_t ld;
    uint32_t n;
    const uint32_t* obs_keys;
    int32_t* obs;
};

__global__ void __launch_bounds__(256) k_predict_logreg(LogregPredictArgs g)
{
    // [k][draw] | [k][row] during the product; afterwards the same bytes hold each wave's logits, half a tile at a time
    __shared__ float smem[D3P_TILE_SMEM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const uint64_t r0 = (uint64_t)blockIdx.x * D3P_TILE_N;
    const uint32_t s0 = blockIdx.y * D3P_TILE_M;
    tile_f16v acc[2][2];
    tile_product(smem, g, r0, s0, acc);
    // Epilogue, per half of the wave's 64 draws: the accumulators go to LDS ([draw 0..31][row 0..63], rows padded to 65 floats), then
    // lane l owns row l and walks the 32 draws -- one threefry call per outcome, 64 consecutive int32 per store.  (Done straight from
    // the accumulator registers, 64 inlined threefry calls per lane make the compiler give up unrolling and index them in scratch.)
    float* L = tile_block(smem);
    const uint64_t r = r0 + wn * 64 + lane;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        tile_scatter(L, acc[mb][0], acc[mb][1]);
        __syncthreads();
        if (r < g.rows) {
            for (int i = 0; i < 32; ++i) {
                const uint32_t s = s0 + wm * 64 + mb * 32 + i;
                if (s >= g.n) break;
                float logit = L[i * 65 + lane];
                if (g.b_col >= 0) logit = logit + g.lat[(size_t)s * g.ld + g.b_col];
                g.obs[(size_t)s * g.rows + r] = bernoulli_draw(tf_iota_word(g.obs_keys[2 * (size_t)s], g.obs_keys[2 * (size_t)s + 1], g.rows, r),
                                                               sigmoid_probs(logit));
            }
        }
        __syncthreads();
    }
}

// ---- Gaussian mean: obs[i, r, c] = Normal(mu_i[c], obs_scale).sample(obs_key_i, (rows, d)); one thread per word pair ----------
__global__ void __launch_bounds__(256) k_predict_gauss(const float* __restrict__ mu, int64_t mu_ld, int d, uint64_t rows, uint32_t n, float obs_scale,
                                                       const uint32_t* __restrict__ obs_keys, float* __restrict__ obs)
{
    const uint64_t size = rows * (uint64_t)d, half = (size + 1) >> 1;
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= half * n) return;
    const uint32_t i = (uint32_t)(q / half);
    const uint64_t j = q - (uint64_t)i * half, j2 = j + half;
    uint32_t wa, wb;
    threefry2x32(obs_keys[2 * (size_t)i], obs_keys[2 * (size_t)i + 1], (uint32_t)j, j2 < size ? (uint32_t)j2 : 0u, wa, wb);
    float* out = obs + (size_t)i * size;
    const float* m = mu + (size_t)i * mu_ld;
    out[j] = normal_site_value(m[j % d], bits_to_normal(wa), obs_scale);
    if (j2 < size) out[j2] = normal_site_value(m[j2 % d], bits_to_normal(wb), obs_scale);
}

// ---- VAE output: obs[i, b, c] = Bernoulli(probs = decoder output).sample(obs_key_i, (B, D)); the decoder ends in a sigmoid,
// here applied to the output layer's pre-activation (logits: n B x D) -----------------------------------------------------------
__global__ void __launch_bounds__(256) k_predict_vae_obs(const float* __restrict__ logits, uint64_t size, uint32_t n, const uint32_t* __restrict__ obs_keys,
                                                         int32_t* __restrict__ obs)
{
    const uint64_t half = (size + 1) >> 1;
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= half * n) return;
    const uint32_t i = (uint32_t)(q / half);
    const uint64_t j = q - (uint64_t)i * half, j2 = j + half;
    uint32_t wa, wb;
    threefry2x32(obs_keys[2 * (size_t)i], obs_keys[2 * (size_t)i + 1], (uint32_t)j, j2 < size ? (uint32_t)j2 : 0u, wa, wb);
    const size_t base = (size_t)i * size;
    obs[base + j] = bernoulli_draw(wa, sigmoid_probs(logits[base + j]));
    if (j2 < size) obs[base + j2] = bernoulli_draw(wb, sigmoid_probs(logits[base + j2]));
}

// (is_device_ptr / D3P_REQUIRE_DEV: d3p_host.h)
static int draws_validate(uint32_t n, int32_t posterior, const d3p_predict_site* sites, int32_t n_sites, int32_t obs_chain, int32_t obs_index,
                          const float* latent, int64_t ld, const uint32_t* obs_keys, const char* what)
{
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n must be >= 1", what);
    if (n_sites < 0 || n_sites > D3P_PREDICT_MAX_SITES) return fail(D3P_E_INVALID_ARG, "%s: 0 <= n_sites <= 8", what);
    if (n_sites > 0 && (!sites || !is_device_ptr(latent))) return fail(D3P_E_INVALID_ARG, "%s: latent_dev must be device memory", what);
    if (n_sites > 0 && (ld < 1 || (uint64_t)n * (uint64_t)ld > (1ull << 40))) return fail(D3P_E_INVALID_ARG, "%s: bad latent_ld", what);
    for (int s = 0; s < n_sites; ++s) {
        const d3p_predict_site& st = sites[s];
        if (st.size < 1 || st.offset < 0 || (int64_t)st.offset + st.size > ld)
            return fail(D3P_E_INVALID_ARG, "%s: site %d does not fit in a latent row", what, s);
        if (st.chain != 0 && !(st.chain == 1 && posterior)) return fail(D3P_E_INVALID_ARG, "%s: site %d: chain 1 (guide) needs posterior", what, s);
        if (st.key_index < -1 || st.key_index > 15) return fail(D3P_E_INVALID_ARG, "%s: site %d: key_index in [-1, 15]", what, s);
        if (st.key_index < 0) {
            if (!is_device_ptr(st.value_dev)) return fail(D3P_E_INVALID_ARG, "%s: site %d: a substituted site needs value_dev in device memory", what, s);
            continue;
        }
        if (st.scale_kind < D3P_PREDICT_SCALE_CONST || st.scale_kind > D3P_PREDICT_SCALE_EXP)
            return fail(D3P_E_INVALID_ARG, "%s: site %d: unknown scale_kind", what, s);
        if ((st.loc_dev && !is_device_ptr(st.loc_dev)) || (st.scale_dev && !is_device_ptr(st.scale_dev)))
            return fail(D3P_E_INVALID_ARG, "%s: site %d: loc / scale must be device memory", what, s);
        if (st.scale_kind != D3P_PREDICT_SCALE_CONST && !st.scale_dev)
            return fail(D3P_E_INVALID_ARG, "%s: site %d: scale_kind needs scale_dev", what, s);
    }
    if (obs_keys) {
        if (!is_device_ptr(obs_keys)) return fail(D3P_E_INVALID_ARG, "%s: obs_keys_dev must be device memory", what);
        if (obs_index < 0 || obs_index > 15) return fail(D3P_E_INVALID_ARG, "%s: obs_index in [0, 15]", what);
        if (obs_chain != 0 && !(obs_chain == 1 && posterior)) return fail(D3P_E_INVALID_ARG, "%s: bad obs_chain", what);
    }
    return D3P_OK;
}

static int draws_enqueue(hipStream_t s, const uint32_t* key, uint32_t n, int32_t multi, int32_t posterior, const d3p_predict_site* sites,
                         int32_t n_sites, int32_t obs_chain, int32_t obs_index, float* latent, int64_t ld, uint32_t* obs_keys)
{
    DrawsArgs a;
    memset(&a, 0, sizeof(a));
    a.key = key; a.n = n; a.multi = multi ? 1 : 0; a.posterior = posterior ? 1 : 0; a.n_sites = n_sites;
    a.obs_chain = obs_chain; a.obs_index = obs_keys ? obs_index : -1;
    uint32_t max_half = 1;
    for (int i = 0; i < n_sites; ++i) {
        a.site[i] = sites[i];
        const uint32_t h = ((uint32_t)sites[i].size + 1) >> 1;
        if (h > max_half) max_half = h;
    }
    a.latent = latent; a.ld = ld; a.obs_keys = obs_keys;
    unsigned gy = cdiv(max_half, 256);
    if (gy > 1024) gy = 1024;
    hipLaunchKernelGGL(k_predict_draws, dim3(n, gy), dim3(256), 0, s, a);
    return check_launch("d3p_predict_draws");
}

// the VAE's dense layer stacks through the product kernels of d3p_gemm.hip (vae_predict_encode / vae_predict_decode: d3p_vae.hip)
int vae_predict_encode(hipStream_t s, const d3p_vae_model* m, const float* params, const float* X, uint32_t B, float* zl, float* zs, float* h0, float* h1,
                       float* sg);
int vae_predict_decode(hipStream_t s, const d3p_vae_model* m, const float* params, const float* z, uint32_t rows, float* logits, float* h0, float* h1,
                       float* sg);

struct VaePredictWs { float *zl, *zs, *h0, *h1, *sg, *logits; uint32_t* obs_keys; };

static size_t vae_predict_carve(const d3p_vae_model* m, uint32_t B, uint32_t n, char* base, VaePredictWs* w)
{
    const size_t R = (size_t)B * n, hmax = (size_t)(m->H > m->H2 ? m->H : m->H2);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) / 256 * 256; return p; };
    VaePredictWs t;
    t.zl = (float*)take((size_t)B * m->Z * 4);
    t.zs = (float*)take((size_t)B * m->Z * 4);
    t.h0 = (float*)take(R * hmax * 4);
    t.h1 = (float*)take(R * hmax * 4);
    t.sg = (float*)take(R * hmax * 4);
    t.logits = (float*)take(R * (size_t)m->D * 4);
    t.obs_keys = (uint32_t*)take((size_t)n * 8);
    if (w) *w = t;
    return off;
}

}  // namespace d3p

using namespace d3p;

extern "C" {

int d3p_predict_draws(void* stream, const uint32_t* key_dev, uint32_t n, int32_t multi, int32_t posterior, const d3p_predict_site* sites_host,
                      int32_t n_sites, int32_t obs_chain, int32_t obs_index, float* latent_dev, int64_t latent_ld, uint32_t* obs_keys_dev)
{
    D3P_REQUIRE_DEV(key_dev, "d3p_predict_draws: key_dev must be device memory");
    if (int rc = draws_validate(n, posterior, sites_host, n_sites, obs_chain, obs_index, latent_dev, latent_ld, obs_keys_dev, "d3p_predict_draws")) return rc;
    if (n_sites == 0 && !obs_keys_dev) return D3P_OK;
    return draws_enqueue((hipStream_t)stream, key_dev, n, multi, posterior, sites_host, n_sites, obs_chain, obs_index, latent_dev, latent_ld, obs_keys_dev);
}

int d3p_predict_logreg(void* stream, const float* X_dev, uint64_t rows, int32_t d, const float* latent_dev, int64_t latent_ld, int32_t w_off,
                       int32_t b_col, uint32_t n, const uint32_t* obs_keys_dev, int32_t* obs_dev)
{
    D3P_REQUIRE(rows >= 1 && rows <= 0xFFFFFFFFull, "d3p_predict_logreg: 1 <= rows <= 2^32 - 1");
    D3P_REQUIRE(d >= 1 && n >= 1, "d3p_predict_logreg: d >= 1 and n >= 1 required");
    D3P_REQUIRE(w_off >= 0 && (int64_t)w_off + d <= latent_ld && b_col < latent_ld && b_col >= -1 && !(b_col >= w_off && b_col < w_off + d),
                "d3p_predict_logreg: the weights [w_off, w_off + d) and the intercept column must lie in a latent row, apart");
    D3P_REQUIRE(cdiv(rows, D3P_TILE_N) <= 0x7fffffffu && cdiv(n, D3P_TILE_M) <= 65535u, "d3p_predict_logreg: grid too large");
    D3P_REQUIRE_DEV(X_dev, "d3p_predict_logreg: X_dev must be device memory");
    D3P_REQUIRE_DEV(latent_dev, "d3p_predict_logreg: latent_dev must be device memory");
    D3P_REQUIRE_DEV(obs_keys_dev, "d3p_predict_logreg: obs_keys_dev must be device memory");
    D3P_REQUIRE_DEV(obs_dev, "d3p_predict_logreg: obs_dev must be device memory");
    LogregPredictArgs g;
    g.X = X_dev; g.rows = rows; g.d = d; g.w_off = w_off; g.b_col = b_col; g.lat = latent_dev; g.ld = latent_ld; g.n = n;
    g.obs_keys = obs_keys_dev; g.obs = obs_dev;
    hipLaunchKernelGGL(k_predict_logreg, dim3(cdiv(rows, D3P_TILE_N), cdiv(n, D3P_TILE_M)), dim3(256), 0, (hipStream_t)stream, g);
    return check_launch("d3p_predict_logreg");
}

int d3p_predict_gauss(void* stream, const float* mu_dev, int64_t mu_ld, int32_t d, uint64_t rows, uint32_t n, float obs_scale,
                      const uint32_t* obs_keys_dev, float* obs_dev)
{
    D3P_REQUIRE(d >= 1 && n >= 1 && rows >= 1 && mu_ld >= d, "d3p_predict_gauss: d, n, rows >= 1 and mu_ld >= d required");
    D3P_REQUIRE(rows * (uint64_t)d <= 0xFFFFFFFFull, "d3p_predict_gauss: rows x d must stay below 2^32 (one threefry stream)");
    D3P_REQUIRE(obs_scale > 0.f, "d3p_predict_gauss: obs_scale must be > 0");
    D3P_REQUIRE_DEV(mu_dev, "d3p_predict_gauss: mu_dev must be device memory");
    D3P_REQUIRE_DEV(obs_keys_dev, "d3p_predict_gauss: obs_keys_dev must be device memory");
    D3P_REQUIRE_DEV(obs_dev, "d3p_predict_gauss: obs_dev must be device memory");
    const uint64_t pairs = ((rows * (uint64_t)d + 1) >> 1) * n;
    D3P_REQUIRE(cdiv(pairs, 256) <= 0x7fffffffu, "d3p_predict_gauss: too many elements");
    hipLaunchKernelGGL(k_predict_gauss, dim3(cdiv(pairs, 256)), dim3(256), 0, (hipStream_t)stream, mu_dev, mu_ld, d, rows, n, obs_scale, obs_keys_dev,
                       obs_dev);
    return check_launch("d3p_predict_gauss");
}

size_t d3p_predict_vae_workspace(const d3p_vae_model* model, uint32_t B, uint32_t n)
{
    if (!model || model->D < 1 || model->H < 1 || model->Z < 1 || model->H2 < 0 || B < 1 || n < 1) return 0;
    return vae_predict_carve(model, B, n, nullptr, nullptr);
}

int d3p_predict_vae(void* stream, const d3p_vae_model* model, const float* params_dev, const float* X_dev, uint32_t B, const uint32_t* key_dev,
                    uint32_t n, int32_t multi, const float* z_subst_dev, float* z_dev, int32_t* obs_dev, void* workspace_dev, size_t workspace_bytes)
{
    D3P_REQUIRE(model && model->D >= 1 && model->H >= 1 && model->Z >= 1 && model->H2 >= 0, "d3p_predict_vae: bad model");
    D3P_REQUIRE(B >= 1 && n >= 1 && (uint64_t)B * n <= 0x7fffffffull, "d3p_predict_vae: 1 <= B, n and n B < 2^31");
    D3P_REQUIRE((uint64_t)B * model->D <= 0xFFFFFFFFull && (uint64_t)B * model->Z <= 0x7fffffffull, "d3p_predict_vae: B too large");
    D3P_REQUIRE((uint64_t)B * n * model->D <= (1ull << 38), "d3p_predict_vae: n B D too large");
    D3P_REQUIRE(!(X_dev && z_subst_dev), "d3p_predict_vae: X_dev (posterior) and z_subst_dev (prior with z substituted) exclude each other");
    D3P_REQUIRE_DEV(key_dev, "d3p_predict_vae: key_dev must be device memory");
    D3P_REQUIRE_DEV(params_dev, "d3p_predict_vae: params_dev must be device memory");
    D3P_REQUIRE_DEV(z_dev, "d3p_predict_vae: z_dev must be device memory");
    D3P_REQUIRE_DEV(obs_dev, "d3p_predict_vae: obs_dev must be device memory");
    D3P_REQUIRE_DEV(workspace_dev, "d3p_predict_vae: workspace_dev must be device memory");
    if (X_dev) D3P_REQUIRE_DEV(X_dev, "d3p_predict_vae: X_dev must be device memory");
    if (z_subst_dev) D3P_REQUIRE_DEV(z_subst_dev, "d3p_predict_vae: z_subst_dev must be device memory");
    if (workspace_bytes < d3p_predict_vae_workspace(model, B, n)) return fail(D3P_E_WORKSPACE, "d3p_predict_vae: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    VaePredictWs w;
    vae_predict_carve(model, B, n, (char*)workspace_dev, &w);
    const int posterior = X_dev ? 1 : 0;
    const int32_t size = (int32_t)(B * (uint32_t)model->Z);
    // the site plan (modelling.site_plan): posterior -- guide: z (guide key 0); model: z substituted by the guide's, obs (model key 0).
    // prior -- model: z (key 0) unless substituted, obs (key 1, or 0 after a substituted z); numpyro.module with its parameters
    // given and the plate of size B with subsample size B take no key
    d3p_predict_site z;
    memset(&z, 0, sizeof(z));
    z.size = size; z.offset = 0;
    z.chain = posterior; z.key_index = z_subst_dev ? -1 : 0;
    z.scale_kind = posterior ? D3P_PREDICT_SCALE_EXP : D3P_PREDICT_SCALE_CONST;
    z.loc_c = 0.f; z.scale_c = 1.f;   // prior: Normal(0, 1) (vae.py:131)
    z.loc_dev = posterior ? w.zl : nullptr;
    z.scale_dev = posterior ? w.zs : nullptr;   // the guide's z_std = exp(Dense(h)) (vae.py:86)
    z.value_dev = z_subst_dev;
    const int32_t obs_index = (posterior || z_subst_dev) ? 0 : 1;
    if (posterior)
        if (int rc = vae_predict_encode(s, model, params_dev, X_dev, B, w.zl, w.zs, w.h0, w.h1, w.sg)) return rc;
    if (int rc = draws_enqueue(s, key_dev, n, multi, posterior, &z, 1, 0, obs_index, z_dev, size, w.obs_keys)) return rc;
    if (int rc = vae_predict_decode(s, model, params_dev, z_dev, B * n, w.logits, w.h0, w.h1, w.sg)) return rc;
    const uint64_t osize = (uint64_t)B * model->D, pairs = ((osize + 1) >> 1) * n;
    hipLaunchKernelGGL(k_predict_vae_obs, dim3(cdiv(pairs, 256)), dim3(256), 0, s, (const float*)w.logits, osize, n, (const uint32_t*)w.obs_keys, obs_dev);
    return check_launch("d3p_predict_vae");
}

}  // extern "C"
