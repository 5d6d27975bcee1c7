// Predictive sampling and cluster assignment of the Gaussian mixture model (d3p_amd/mixture.py): the latent
// draws of n prior or posterior draws, the n x rows x d outcomes of the observed site, and the per-component log-posterior of given
// points with its argmax.
//
// The key rule is section 4b's (d3p_predict.hip), restated here because that file's text is pinned: draw i runs on split(key, n)[i]
// (the single form on the key itself); the prior seeds the model's chain with the draw's key, the posterior splits it into the
// model's and the guide's chain; every key-taking sample statement does `chain, site_key = split(chain)` in program order pis, mus,
// sigs (guide or model) and then obs (model).  A site whose value is given is copied in and takes no key, so the later sites' keys
// shift: d3p_predict_gmm_draws counts the key indices from which value pointers are null (index -1: substituted).
// tests/mixture_ref.py restates the same plan on the host, and the GPU tests hold the two against each other.
//
// Site rules, one device function each:
//   pgm_gamma_sample   the project's own Gamma(alpha, 1) draw (Marsaglia-Tsang on the site key's threefry words, float64): a SECOND
//                      COPY of gamma_sample_d (d3p_gmm.hip), on purpose -- that file's text is measured and pinned, and moving the
//                      function into a header changed its kernels' generated code; unifying the copies is a refactor of its own.
//                      pis_j = (float)(g_j / sum g), the sum in index order.  No bit parity with jax.random.gamma is claimed.
//   pgm_normal_value   numpyro Normal.sample: loc + normal * scale, a product, then a sum (normal_site_value's rule)
//   pgm_inverse_gamma  InverseGamma(1, 1) by inversion: 1 / -logf(u), u = ((bits >> 9) + 0.5) 2^-23 (the rule of k_gmm_eval_latents)
//   pgm_component      GaussianMixture.sample_with_intermediates (d3p/gmm.py:91-95): z = min(#{j : cum_j < u}, k - 1) with cum the
//                      float32 running sum of pis taken left to right
//
// k_predict_gmm_obs is the hot path.  jax lays normal(samples_key, (rows, d)) out as threefry(key, iota(rows d)) split in two halves:
// ONE threefry call yields elements e and e + H, H = ceil(rows d / 2).  A workgroup therefore owns D3P_PGM_TP d consecutive PAIRS:
// the elements [P0, P0 + TP d) of the lower half -- whole rows, TP of them -- and their partners [P0 + H, P0 + H + TP d) of the upper
// half, which touch at most TP + 1 rows.  Both words of every call are used, whatever the shape; a workgroup covers
// D3P_PGM_ROW_TILE = 2 TP rows of the output.  Lane l of a wave walks pairs l, l + 256, ...: a store is 64 consecutive floats of the
// row-major (rows, d) output, in the lower and in the upper range alike.  u, z and eps never reach memory (z only through zs_out).
#include "d3p_colreduce.h"
#include "d3p_device.h"

namespace d3p {

#define D3P_PGM_TP 64
#define D3P_PGM_ROW_TILE (2 * D3P_PGM_TP)
#define D3P_PGM_MAX_K 32
#define D3P_PGM_MAX_KD 4096   // k <= 16 with d <= 256, or k <= 32 with d <= 128

// jax.random.split(key) (two children): words 0..3 of threefry_2x32(key, iota(4)) -> child 0 = (w0, w1), child 1 = (w2, w3)
__device__ __forceinline__ void pgm_split2(uint32_t k0, uint32_t k1, uint32_t& a0, uint32_t& a1, uint32_t& b0, uint32_t& b1)
{
    threefry2x32(k0, k1, 0u, 2u, a0, b0);
    threefry2x32(k0, k1, 1u, 3u, a1, b1);
}

// numpyro.handlers.seed: `rng, site_key = split(rng)` at every key-taking sample statement; index = how many came before
__device__ __forceinline__ void pgm_site_key(uint32_t c0, uint32_t c1, int index, uint32_t& s0, uint32_t& s1)
{
    for (int j = 0; j <= index; ++j) {
        uint32_t n0, n1;
        pgm_split2(c0, c1, n0, n1, s0, s1);
        c0 = n0; c1 = n1;
    }
}

__device__ __forceinline__ double pgm_open_unit(uint32_t b) { return ((double)b + 0.5) * (1.0 / 4294967296.0); }

// gamma_sample_d of d3p_gmm.hip, word for word (file comment)
__device__ __forceinline__ double pgm_gamma_sample(uint32_t k0, uint32_t k1, uint32_t comp, double alpha)
{
    if (!(alpha < 1.7976931348623157e308)) return alpha;
    const double a = alpha < 1.0 ? alpha + 1.0 : alpha;
    const double dd = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * dd);
    double g = 0.0;
    for (uint32_t attempt = 0; attempt < 1024u; ++attempt) {
        uint32_t b0, b1;
        threefry2x32(k0, k1, comp, attempt, b0, b1);
        const double x = (double)bits_to_normal(b0);
        const double U = pgm_open_unit(b1);
        const double v1 = 1.0 + c * x;
        if (v1 <= 0.0) continue;
        const double v = v1 * v1 * v1;
        if (log(U) < 0.5 * x * x + dd - dd * v + dd * log(v)) { g = dd * v; break; }
    }
    if (alpha < 1.0) {
        uint32_t b0, b1;
        threefry2x32(k0, k1, comp, 0x80000000u, b0, b1);
        g *= pow(pgm_open_unit(b0), 1.0 / alpha);
    }
    return g;
}

// The pragma keeps hipcc from contracting the product and the sum into one fma (tests/test_gpu_mixture.py checks the two roundings)
__device__ __forceinline__ float pgm_normal_value(float loc, float eps, float scale)
{
#pragma clang fp contract(off)
    return loc + eps * scale;
}

__device__ __forceinline__ float pgm_inverse_gamma(uint32_t bits)
{
    const float ex = -logf(((float)(bits >> 9) + 0.5f) * 1.1920928955078125e-07f);
    return 1.0f / ex;
}

__device__ __forceinline__ int pgm_component(const float* cum, int k, float u)
{
    int z = 0;
    for (int j = 0; j < k; ++j) z += cum[j] < u ? 1 : 0;
    return z < k - 1 ? z : k - 1;
}

// ---- latent draws: one workgroup per draw writes its row [pis (k) | mus (k d) | sigs (k d)] and its obs key -----------------------
struct GmmDrawsArgs {
    const uint32_t* key;
    uint32_t n;
    int multi, posterior, k, d;
    int idx_pis, idx_mus, idx_sigs, idx_obs;   // key indices under the latent sites' chain / the model's chain; -1: substituted
    const float* alpha_log;                    // posterior
    const float* mus_loc;                      // posterior
    float prior_mu_scale;
    const float* pis_v;
    const float* mus_v;
    const float* sigs_v;
    float* lat;
    uint32_t* obs_keys;
};

__global__ void __launch_bounds__(256) k_predict_gmm_draws(GmmDrawsArgs a)
{
    __shared__ double g_s[D3P_PGM_MAX_K];
    const uint32_t i = blockIdx.x;
    const int tid = threadIdx.x, k = a.k;
    const uint32_t kd = (uint32_t)(a.k * a.d);
    // modelling._sample_a_lot: draw i of the multi form runs on split(key, n)[i]
    uint32_t d0 = a.key[0], d1 = a.key[1];
    if (a.multi) {
        const uint32_t q0 = d0, q1 = d1;
        d0 = tf_iota_word(q0, q1, 2ull * a.n, 2ull * i);
        d1 = tf_iota_word(q0, q1, 2ull * a.n, 2ull * i + 1);
    }
    // modelling.sample_posterior_predictive: model_key, guide_key = split(key); the prior seeds the model with the key itself
    uint32_t m0 = d0, m1 = d1, l0 = d0, l1 = d1;   // the model's chain; the chain of the latent sites
    if (a.posterior) pgm_split2(d0, d1, m0, m1, l0, l1);
    if (tid == 0) {
        uint32_t s0, s1;
        pgm_site_key(m0, m1, a.idx_obs, s0, s1);
        a.obs_keys[2 * (size_t)i] = s0;
        a.obs_keys[2 * (size_t)i + 1] = s1;
    }
    float* row = a.lat + (size_t)i * (size_t)(k + 2 * kd);
    if (a.idx_pis < 0) {
        if (tid < k) row[tid] = a.pis_v[tid];
    } else {
        uint32_t s0, s1;
        pgm_site_key(l0, l1, a.idx_pis, s0, s1);
        if (tid < k) g_s[tid] = pgm_gamma_sample(s0, s1, (uint32_t)tid, a.posterior ? exp((double)a.alpha_log[tid]) : 1.0);
        __syncthreads();
        double S = 0.0;
        for (int j = 0; j < k; ++j) S += g_s[j];   // index order
        if (tid < k) row[tid] = (float)(g_s[tid] / S);
    }
    const uint32_t half = (kd + 1) >> 1;
    float* mus = row + k;
    if (a.idx_mus < 0) {
        for (uint32_t j = tid; j < kd; j += 256) mus[j] = a.mus_v[j];
    } else {
        uint32_t s0, s1;
        pgm_site_key(l0, l1, a.idx_mus, s0, s1);
        for (uint32_t j = tid; j < half; j += 256) {
            const uint32_t j2 = j + half;
            uint32_t wa, wb;
            threefry2x32(s0, s1, j, j2 < kd ? j2 : 0u, wa, wb);
            mus[j] = a.posterior ? pgm_normal_value(a.mus_loc[j], bits_to_normal(wa), 1.0f)
                                 : pgm_normal_value(0.0f, bits_to_normal(wa), a.prior_mu_scale);
            if (j2 < kd)
                mus[j2] = a.posterior ? pgm_normal_value(a.mus_loc[j2], bits_to_normal(wb), 1.0f)
                                      : pgm_normal_value(0.0f, bits_to_normal(wb), a.prior_mu_scale);
        }
    }
    float* sigs = mus + kd;
    if (a.idx_sigs < 0) {
        for (uint32_t j = tid; j < kd; j += 256) sigs[j] = a.sigs_v[j];
    } else {
        uint32_t s0, s1;
        pgm_site_key(l0, l1, a.idx_sigs, s0, s1);
        for (uint32_t j = tid; j < half; j += 256) {
            const uint32_t j2 = j + half;
            uint32_t wa, wb;
            threefry2x32(s0, s1, j, j2 < kd ? j2 : 0u, wa, wb);
            sigs[j] = pgm_inverse_gamma(wa);
            if (j2 < kd) sigs[j2] = pgm_inverse_gamma(wb);
        }
    }
}

// ---- outcomes: grid (pair tiles, draws) --------------------------------------------------------------------------------------------
struct GmmObsArgs {
    const float* lat;
    int64_t ld;
    int k, d;
    uint32_t rows, n_tot, half;   // n_tot = rows d < 2^32, half = ceil(n_tot / 2)
    const uint32_t* obs_keys;
    float* obs;
    int32_t* zs;
};

__global__ void __launch_bounds__(256) k_predict_gmm_obs(GmmObsArgs g)
{
    // mus / sigs rows of component z are read at z d + c: lanes of one output row read consecutive words (no bank conflict); lanes of
    // different rows with different z may meet on a bank (d < 32 only), identical addresses broadcast
    // (the 33 KB are static whatever k d is: 4 workgroups per CU at most, also for a small mixture; and a tile of TP d pairs leaves
    // lanes without a pair when d < 4 -- 128 of the 256 threads walk at d = 2, 64 at d = 1.  Both unmeasured: DESIGN.md section 4f)
    __shared__ float mus_s[D3P_PGM_MAX_KD], sigs_s[D3P_PGM_MAX_KD], cum_s[D3P_PGM_MAX_K];
    __shared__ uint32_t key_s[4];
    __shared__ uint8_t z_s[2][D3P_PGM_TP + 4];   // [0]: the TP rows of the lower range, [1]: the <= TP + 1 rows of the upper range
    const int tid = threadIdx.x, k = g.k, d = g.d;
    const uint32_t s = blockIdx.y, kd = (uint32_t)(k * d);
    const float* row = g.lat + (size_t)s * g.ld;
    for (uint32_t j = tid; j < kd; j += 256) {
        mus_s[j] = row[k + j];
        sigs_s[j] = row[k + kd + j];
    }
    if (tid == 0) {
        float c = 0.f;
        for (int j = 0; j < k; ++j) { c = c + row[j]; cum_s[j] = c; }   // np.cumsum(float32): left to right
        // component_key, samples_key = split(obs_key)
        pgm_split2(g.obs_keys[2 * (size_t)s], g.obs_keys[2 * (size_t)s + 1], key_s[0], key_s[1], key_s[2], key_s[3]);
    }
    __syncthreads();
    const uint32_t tile = D3P_PGM_TP * (uint32_t)d;        // pairs per workgroup (<= 16384)
    const uint32_t P0 = blockIdx.x * tile;                 // < half <= 2^31
    const uint32_t np = g.half - P0 < tile ? g.half - P0 : tile;
    const uint32_t eu0 = P0 + g.half;                      // first element of the upper range (<= 2^32 - 1)
    const uint64_t rl0 = (uint64_t)blockIdx.x * D3P_PGM_TP, ru0 = eu0 / (uint32_t)d;
    if (tid < 2 * D3P_PGM_TP + 1) {
        const int hi = tid >= D3P_PGM_TP, i = hi ? tid - D3P_PGM_TP : tid;
        const uint64_t r = (hi ? ru0 : rl0) + (uint64_t)i;
        if (r < g.rows) {
            // u = uniform(component_key, (rows, 1))[r]
            const float u = bits_to_uniform(tf_iota_word(key_s[0], key_s[1], g.rows, r), 0.0f, 1.0f);
            const int z = pgm_component(cum_s, k, u);
            z_s[hi][i] = (uint8_t)z;
            // a row is written by the range that holds its first element
            const uint64_t e = r * (uint64_t)d;
            const bool mine = hi ? (e >= eu0 && e < (uint64_t)eu0 + np) : (e < g.half);
            if (g.zs && mine) g.zs[(size_t)s * g.rows + r] = z;
        }
    }
    __syncthreads();
    const uint32_t m0 = key_s[2], m1 = key_s[3];
    const uint32_t cu0 = eu0 - (uint32_t)ru0 * (uint32_t)d;
    uint32_t rl = (uint32_t)tid / (uint32_t)d, cl = (uint32_t)tid % (uint32_t)d;
    uint32_t ru = (cu0 + (uint32_t)tid) / (uint32_t)d, cu = (cu0 + (uint32_t)tid) % (uint32_t)d;
    const uint32_t qs = 256u / (uint32_t)d, rs = 256u % (uint32_t)d;
    float* out = g.obs + (size_t)s * g.n_tot;
    for (uint32_t p = tid; p < np; p += 256) {
        const uint32_t e0 = P0 + p, e1 = e0 + g.half;
        const bool has1 = e1 < g.n_tot;
        uint32_t w0, w1;
        threefry2x32(m0, m1, e0, has1 ? e1 : 0u, w0, w1);
        {
            const uint32_t j = (uint32_t)z_s[0][rl] * (uint32_t)d + cl;
            out[e0] = pgm_normal_value(mus_s[j], bits_to_normal(w0), sigs_s[j]);
        }
        if (has1) {
            const uint32_t j = (uint32_t)z_s[1][ru] * (uint32_t)d + cu;
            out[e1] = pgm_normal_value(mus_s[j], bits_to_normal(w1), sigs_s[j]);
        }
        cl += rs; rl += qs;
        if (cl >= (uint32_t)d) { cl -= (uint32_t)d; ++rl; }
        cu += rs; ru += qs;
        if (cu >= (uint32_t)d) { cu -= (uint32_t)d; ++ru; }
    }
}

// ---- assignment: a[r, j] = log pis_j + sum_c log N(x_rc; mus_jc, sigs_jc), the tile of k_gmm_log_prob (d3p_stages.hip) -------------
// One wavefront per row; lanes stride the event dimension (a lane's terms in index order), the k component sums go through the
// fixed-order wave reduction.  The DIRECT form ((x - mu) / sig)^2: the expanded x^2 a - 2 x b + c cancels about four digits at scales
// near 0.06 and |x| near 10, so this is not a matrix product.
template <int KMAX>
__global__ void __launch_bounds__(256) k_gmm_assign(const float* __restrict__ x, uint64_t rows, int d, const float* __restrict__ mus,
                                                    const float* __restrict__ sigs, const float* __restrict__ pis, int k,
                                                    float* __restrict__ a_out, int32_t* __restrict__ arg_out)
{
    const uint64_t r = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;   // (wave-uniform)
    float comp[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) comp[j] = 0.f;
    for (int c = lane; c < d; c += 64) {
        const float xv = x[r * (uint64_t)d + c];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j < k) {
                const float sc = sigs[(size_t)j * d + c];
                const float z = (xv - mus[(size_t)j * d + c]) / sc;
                comp[j] += -0.5f * z * z - logf(sc) - D3P_HALF_LOG_2PI;
            }
        }
    }
    float best = -INFINITY, mine = 0.f;
    int arg = 0;
    bool nan = false;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        if (j < k) {
            const float v = wave_sum(comp[j]) + logf(pis[j]);
            nan |= v != v;
            if (v > best) { best = v; arg = j; }   // first maximum on ties
            if (lane == j) mine = v;
        }
    }
    if (nan) { mine = __builtin_nanf(""); arg = -1; }   // a NaN anywhere in the row: the whole row is NaN, no assignment
    if (a_out && lane < k) a_out[r * (uint64_t)k + lane] = mine;
    if (arg_out && lane == 0) arg_out[r] = arg;
}

static int pgm_limits(int32_t k, int32_t d, const char* what)
{
    if (k < 1 || d < 1) return fail(D3P_E_INVALID_ARG, "%s: k and d must be >= 1 (k = %d, d = %d)", what, k, d);
    if (k > 32 || d > 256 || (k > 16 && d > 128))
        return fail(D3P_E_UNSUPPORTED, "%s: supported shapes are k <= 16 with d <= 256 and k <= 32 with d <= 128 (k = %d, d = %d)", what, k, d);
    return D3P_OK;
}


}  // namespace d3p

using namespace d3p;

extern "C" {

int d3p_predict_gmm_draws(void* stream, const uint32_t* key_dev, uint32_t n, int32_t multi, int32_t posterior, int32_t k, int32_t d,
                          const float* alpha_log_dev, const float* mus_loc_dev, float prior_mu_scale, const float* pis_value_dev,
                          const float* mus_value_dev, const float* sigs_value_dev, float* latent_dev, uint32_t* obs_keys_dev)
{
    const char* what = "d3p_predict_gmm_draws";
    if (!key_dev || !latent_dev || !obs_keys_dev) return fail(D3P_E_INVALID_ARG, "%s: null key / latent / obs_keys pointer", what);
    if (!aligned4(key_dev) || !aligned4(latent_dev) || !aligned4(obs_keys_dev) || !aligned4(alpha_log_dev) ||
        !aligned4(mus_loc_dev) || !aligned4(pis_value_dev) || !aligned4(mus_value_dev) || !aligned4(sigs_value_dev))
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (int rc = pgm_limits(k, d, what)) return rc;
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n must be >= 1", what);
    if (!multi && n != 1) return fail(D3P_E_INVALID_ARG, "%s: the single form draws once (n = %u)", what, n);
    if (n > 0x7fffffffu) return fail(D3P_E_UNSUPPORTED, "%s: n <= 2^31 - 1", what);
    if (posterior) {
        if (!alpha_log_dev || !mus_loc_dev) return fail(D3P_E_INVALID_ARG, "%s: the posterior needs alpha_log and mus_loc", what);
        if (pis_value_dev || mus_value_dev || sigs_value_dev)
            return fail(D3P_E_INVALID_ARG, "%s: substituted sites are a prior-predictive argument", what);
    } else if (!(prior_mu_scale > 0.f)) {
        return fail(D3P_E_INVALID_ARG, "%s: prior_mu_scale must be > 0", what);
    }
    if (!is_device_ptr(key_dev) || !is_device_ptr(latent_dev) || !is_device_ptr(obs_keys_dev) ||
        (posterior && (!is_device_ptr(alpha_log_dev) || !is_device_ptr(mus_loc_dev))) || (pis_value_dev && !is_device_ptr(pis_value_dev)) ||
        (mus_value_dev && !is_device_ptr(mus_value_dev)) || (sigs_value_dev && !is_device_ptr(sigs_value_dev)))
        return fail(D3P_E_INVALID_ARG, "%s: every pointer must be device memory", what);
    GmmDrawsArgs a;
    a.key = key_dev; a.n = n; a.multi = multi != 0; a.posterior = posterior != 0; a.k = k; a.d = d;
    int next = 0;   // program order pis, mus, sigs under the latent sites' chain; a substituted site takes no key
    a.idx_pis = pis_value_dev ? -1 : next++;
    a.idx_mus = mus_value_dev ? -1 : next++;
    a.idx_sigs = sigs_value_dev ? -1 : next++;
    a.idx_obs = posterior ? 0 : next;   // the posterior's latents are substituted into the model: obs takes its chain's key 0
    a.alpha_log = alpha_log_dev; a.mus_loc = mus_loc_dev; a.prior_mu_scale = prior_mu_scale;
    a.pis_v = pis_value_dev; a.mus_v = mus_value_dev; a.sigs_v = sigs_value_dev;
    a.lat = latent_dev; a.obs_keys = obs_keys_dev;
    hipLaunchKernelGGL(k_predict_gmm_draws, dim3(n), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch(what);
}

int d3p_predict_gmm_obs(void* stream, const float* latent_dev, int64_t latent_ld, int32_t k, int32_t d, uint64_t rows, uint32_t n,
                        const uint32_t* obs_keys_dev, float* obs_dev, int32_t* zs_out_dev)
{
    const char* what = "d3p_predict_gmm_obs";
    if (!latent_dev || !obs_keys_dev || !obs_dev) return fail(D3P_E_INVALID_ARG, "%s: null latent / obs_keys / obs pointer", what);
    if (!aligned4(latent_dev) || !aligned4(obs_keys_dev) || !aligned4(obs_dev) || !aligned4(zs_out_dev))
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (int rc = pgm_limits(k, d, what)) return rc;
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n must be >= 1", what);
    if (latent_ld < (int64_t)k + 2 * (int64_t)k * d) return fail(D3P_E_INVALID_ARG, "%s: a latent row holds k + 2 k d values", what);
    if (rows > 0xFFFFFFFFull || rows * (uint64_t)d > 0xFFFFFFFFull)
        return fail(D3P_E_UNSUPPORTED, "%s: rows d < 2^32 (one threefry stream of rows d normals per draw)", what);
    if (rows == 0) return D3P_OK;
    if (!is_device_ptr(latent_dev) || !is_device_ptr(obs_keys_dev) || !is_device_ptr(obs_dev) || (zs_out_dev && !is_device_ptr(zs_out_dev)))
        return fail(D3P_E_INVALID_ARG, "%s: latent, obs_keys, obs and zs_out must be device memory", what);
    GmmObsArgs g;
    g.ld = latent_ld; g.k = k; g.d = d; g.rows = (uint32_t)rows; g.n_tot = (uint32_t)(rows * (uint64_t)d);
    g.half = (uint32_t)(((uint64_t)g.n_tot + 1) >> 1);
    const unsigned tiles = cdiv(g.half, (uint64_t)D3P_PGM_TP * d);
    // the draws are the grid's y dimension (at most 65535 per launch): more draws go out in several launches
    for (uint32_t s0 = 0; s0 < n; s0 += 65535u) {
        const uint32_t ns = n - s0 < 65535u ? n - s0 : 65535u;
        g.lat = latent_dev + (size_t)s0 * (size_t)latent_ld;
        g.obs_keys = obs_keys_dev + 2 * (size_t)s0;
        g.obs = obs_dev + (size_t)s0 * g.n_tot;
        g.zs = zs_out_dev ? zs_out_dev + (size_t)s0 * g.rows : nullptr;
        hipLaunchKernelGGL(k_predict_gmm_obs, dim3(tiles, ns), dim3(256), 0, (hipStream_t)stream, g);
    }
    return check_launch(what);
}

int d3p_gmm_assign(void* stream, const float* obs_dev, uint64_t rows, int32_t d, const float* mus_dev, const float* sigs_dev,
                   const float* pis_dev, int32_t k, float* a_out_dev, int32_t* argmax_out_dev)
{
    const char* what = "d3p_gmm_assign";
    if (!obs_dev || !mus_dev || !sigs_dev || !pis_dev) return fail(D3P_E_INVALID_ARG, "%s: null obs / mus / sigs / pis pointer", what);
    if (!a_out_dev && !argmax_out_dev) return fail(D3P_E_INVALID_ARG, "%s: at least one of the two outputs is required", what);
    if (!aligned4(obs_dev) || !aligned4(mus_dev) || !aligned4(sigs_dev) || !aligned4(pis_dev) || !aligned4(a_out_dev) ||
        !aligned4(argmax_out_dev))
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (int rc = pgm_limits(k, d, what)) return rc;
    if (rows > 0xFFFFFFFFull || rows * (uint64_t)d > 0xFFFFFFFFull) return fail(D3P_E_UNSUPPORTED, "%s: rows d < 2^32", what);
    if (rows == 0) return D3P_OK;
    if (!is_device_ptr(obs_dev) || !is_device_ptr(mus_dev) || !is_device_ptr(sigs_dev) || !is_device_ptr(pis_dev) ||
        (a_out_dev && !is_device_ptr(a_out_dev)) || (argmax_out_dev && !is_device_ptr(argmax_out_dev)))
        return fail(D3P_E_INVALID_ARG, "%s: every pointer must be device memory", what);
    const dim3 grid(cdiv(rows * 64, 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (k <= 4)
        hipLaunchKernelGGL(k_gmm_assign<4>, grid, block, 0, s, obs_dev, rows, d, mus_dev, sigs_dev, pis_dev, k, a_out_dev, argmax_out_dev);
    else if (k <= 16)
        hipLaunchKernelGGL(k_gmm_assign<16>, grid, block, 0, s, obs_dev, rows, d, mus_dev, sigs_dev, pis_dev, k, a_out_dev, argmax_out_dev);
    else
        hipLaunchKernelGGL(k_gmm_assign<32>, grid, block, 0, s, obs_dev, rows, d, mus_dev, sigs_dev, pis_dev, k, a_out_dev, argmax_out_dev);
    return check_launch(what);
}

}  // extern "C"
