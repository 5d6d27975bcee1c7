// DP-VI step for the variational auto-encoder of BASELINE config 5 (examples/vae.py:65-153): the one place on the
// path where the model forward is a dense layer stack, so the per-example gradient work is GEMM-shaped and runs on
// the matrix cores (fp32 MFMA, v_mfma_f32_32x32x2_f32; the reference computes in float32 throughout).
//
// The B x P per-example gradient tensor (P = 688 884) is never formed:
//   * a dense layer y = a W + b has per-example gradients  dW_i = a_i d_i^T, db_i = d_i, so
//     ||dW_i||_F^2 + ||db_i||^2 = (||a_i||^2 + 1) ||d_i||^2   -> the joint L2 norm needs only row norms;
//   * the clipped sum  sum_i c_i a_i d_i^T = A^T (diag(c) Delta)  is one GEMM per layer.
// Forward and backward-data passes are batched GEMMs over the B examples; activations, the reparametrised latent,
// the Bernoulli likelihood and the clip factors are small row-wise kernels in between.
// The products themselves -- kernels, routing rule, dispatcher gemm(), grouped launch -- are d3p_gemm.hip / d3p_gemm.h; this file is
// the model: stages, VaeNet, workspace, forward / sums / predictive passes, C entries and the data-parallel run.
// Formulas: oracle/d3p_oracle.c (d3po_vae_step_sums), which materialises every per-example gradient as the check.
#include "d3p_gemm.h"
#include "d3p_fmesh.h"
#include <mutex>
#include <unordered_map>
#include <map>
#include <utility>

namespace d3p {

static inline size_t align_up_v(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The run loop's batch: rows idx[0 .. B - 1] of the resident table gathered into xb (what d3p_take_rows does) AND the exactness
// pass over them in the same sweep (the batch is read once instead of twice).  d4 = row length in 16-byte words.
__global__ void __launch_bounds__(256) k_vae_gather_check(const float* __restrict__ table, const uint32_t* __restrict__ idx, uint32_t B, uint32_t d4,
                                                          float* __restrict__ xb, uint32_t* __restrict__ flag, uint32_t nonce)
{
    uint32_t bad = 0u;
    const size_t n = (size_t)B * d4;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(e / d4), c = (uint32_t)(e % d4);
        const uint4 v = reinterpret_cast<const uint4*>(table)[(size_t)idx[row] * d4 + c];
        reinterpret_cast<uint4*>(xb)[e] = v;
        bad |= (v.x | v.y | v.z | v.w) & 0xffffu;
    }
    if (flag && __ballot(bad != 0u) != 0ull && (threadIdx.x & 63) == 0) *flag = nonce;
}

// ------------------------------------------------------------------------------------------------------------------
// row-wise / element-wise stages
// ------------------------------------------------------------------------------------------------------------------
// DPSVI.evaluate: ONE guide draw for the whole batch -- eps = normal(k_z, (B, Z)) with
// rng_key_eval = split(key)[1], guide_seed = split(.)[1], k_z = split(.)[1]  (numpyro SVI.evaluate / Trace_ELBO / seed handler)
__global__ void k_vae_eval_eps(const uint32_t* __restrict__ jax_key, uint32_t B, int Z, float* __restrict__ eps)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)B * Z;
    if (t >= n) return;
    uint32_t k0 = jax_key[0], k1 = jax_key[1];
#pragma unroll
    for (int lvl = 0; lvl < 3; ++lvl) {
        uint32_t a, b0, b1;
        threefry2x32(k0, k1, 0u, 2u, a, b0);
        threefry2x32(k0, k1, 1u, 3u, a, b1);
        k0 = b0;
        k1 = b1;
    }
    eps[t] = bits_to_normal(tf_iota_word(k0, k1, (uint64_t)n, (uint64_t)t));
}

// Gaussian-mechanism noise for all parameter leaves (10, or 14 with two hidden layers) in one launch: leaf k draws
// normal(site_key_k, leaf shape) (svi.py:487-491), i.e. word w of ChaCha block b of key k is element 16 b + w of that leaf.
#define D3P_VAE_MAX_LEAVES 14 // parameter leaves: 2 (2 nh + 1) + 4
struct SiteNoiseArgs {
    const uint32_t* site_keys;                    // n_leaves x 16
    uint32_t blk_off[D3P_VAE_MAX_LEAVES + 1];     // prefix sums of ceil(leaf size / 16) (unused entries = the total)
    uint32_t elem_off[D3P_VAE_MAX_LEAVES + 1];    // prefix sums of the leaf sizes
    float* noise;
};

__device__ __forceinline__ void site_noise_block(const SiteNoiseArgs& a, uint32_t b)   // b = ChaCha block over all leaves
{
    if (b >= a.blk_off[D3P_VAE_MAX_LEAVES]) return;
    int site = 0;
#pragma unroll
    for (int k = 1; k < D3P_VAE_MAX_LEAVES; ++k) site += (b >= a.blk_off[k]) ? 1 : 0;
    const uint32_t lb = b - a.blk_off[site], n_site = a.elem_off[site + 1] - a.elem_off[site];
    uint32_t key[16], o[16];
    load_key(a.site_keys + 16 * site, key);
    keystream_block(key, lb, o);
    float* dst = a.noise + a.elem_off[site];
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const uint32_t e = 16u * lb + w;
        if (e < n_site) dst[e] = bits_to_normal(o[w]);
    }
}

__global__ void __launch_bounds__(256) k_vae_site_noise(SiteNoiseArgs a) { site_noise_block(a, blockIdx.x * blockDim.x + threadIdx.x); }

// zl, u (B x Z), eps -> z = zl + exp(u) eps (written over zl), sd = exp(u) (written over u), lat[i] = log q - log p
// (zl / u, like dz / du below, are the two halves of one B x 2 Z array: row stride ld)
// jax_key != nullptr: the guide noise is drawn here -- eps[i][j] = normal word j of example i's sample key (svi.py:289-290;
// single site 'z'; the key of an example is a function of its GLOBAL position pos0 + i in a batch of B_total, so 1 GPU and N
// GPUs draw the same noise) -- and written to eps_out for the backward pass; otherwise eps_in is used (tests, evaluate).
// splits > 0: [zl | u] has not been written yet -- the product h [Wl | Ws] left `splits` split-K partial tiles in part
// ([split][B][2 Z]); they are summed here in the order and with the bias addition of k_gemm_reduce (which this replaces).
// noise_blocks > 0: the first noise_blocks workgroups of the launch draw the Gaussian-mechanism noise of the update instead
// (site_noise_block: needs the step's keys only, so it rides in this short launch instead of one of its own).
struct LatentArgs {
    float *zl, *u;
    const float* eps_in;
    const uint32_t* jax_key;
    uint32_t B_total, pos0;
    float* eps_out;
    uint32_t B;
    int Z, ld;
    float* lat;
    const float* part;
    int splits;
    const float *bias_l, *bias_s;
    unsigned noise_blocks;
    SiteNoiseArgs noise;
};

__global__ void __launch_bounds__(256) k_vae_latent(LatentArgs a)
{
    if (blockIdx.x < a.noise_blocks) {
        site_noise_block(a.noise, blockIdx.x * blockDim.x + threadIdx.x);
        return;
    }
    const uint32_t i = ((blockIdx.x - a.noise_blocks) * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= a.B) return;
    const int Z = a.Z;
    uint32_t k0 = 0, k1 = 0;
    if (a.jax_key) px_sample_key(a.jax_key[0], a.jax_key[1], a.B_total, a.pos0 + i, k0, k1);
    float acc = 0.f;
    for (int j = lane; j < Z; j += 64) {
        const size_t e = (size_t)i * a.ld + j;
        float ee;
        if (a.jax_key) {
            ee = bits_to_normal(tf_iota_word(k0, k1, (uint64_t)Z, (uint64_t)j));
            a.eps_out[(size_t)i * Z + j] = ee;
        } else {
            ee = a.eps_in[(size_t)i * Z + j];
        }
        float loc, uu;
        if (a.splits > 0) {
            const size_t tile = (size_t)a.B * 2 * Z, t = (size_t)i * 2 * Z + j;
            float sl = 0.f, su = 0.f;
            for (int z = 0; z < a.splits; ++z) { sl += a.part[z * tile + t]; su += a.part[z * tile + t + Z]; }  // fixed order
            loc = __fmaf_rn(1.0f, sl, a.bias_l[j]);
            uu = __fmaf_rn(1.0f, su, a.bias_s[j]);
        } else {
            loc = a.zl[e];
            uu = a.u[e];
        }
        const float sd = expf(uu), z = __fmaf_rn(sd, ee, loc);
        a.zl[e] = z;
        a.u[e] = sd;
        acc += (-0.5f * ee * ee - uu) + 0.5f * z * z;  // the log(2 pi) / 2 terms of log q and log p cancel
    }
    acc = wave_sum(acc);
    if (lane == 0) a.lat[i] = acc;
}

// logits a (B x D), x -> da = sc (sigmoid(a) - x) in place; px_loss[i] = sc (lat_i - sum_j (x a - softplus(a))) mask_i
// (also leaves x2[i] = |x_i|^2 for the norm kernel, which then need not read X again)
__global__ void k_vae_out(float* __restrict__ a, const float* __restrict__ X, const uint8_t* __restrict__ mask, uint32_t B, int D,
                          float sc, const float* __restrict__ lat, float* __restrict__ px_loss, float* __restrict__ x2)
{
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= B) return;
    // one exponential per element: e = exp(-|t|) gives softplus(t) = max(t, 0) + log1p(e) and sigmoid(t) = 1 / (1 + e) for
    // t >= 0, e / (1 + e) otherwise
    float xx = 0.f;
    auto elem = [&](float t, float x, float& ll) {
        xx = __fmaf_rn(x, x, xx);
        // (hardware exp2 / log2 / rcp paths: 1 + e is in (1, 2], so log(1 + e) has an absolute error of ~1e-7 against terms >= ln 2 e)
        const float e = __expf(-fabsf(t)), r = __builtin_amdgcn_rcpf(1.0f + e);
        ll += x * t - (fmaxf(t, 0.0f) + __logf(1.0f + e));
        return sc * ((t >= 0.0f ? r : e * r) - x);
    };
    float ll = 0.f;
    float* ar = a + (size_t)i * D;
    const float* xr = X + (size_t)i * D;
    if ((D & 3) == 0 && ((reinterpret_cast<uintptr_t>(ar) | reinterpret_cast<uintptr_t>(xr)) & 15u) == 0) {
        for (int j = 4 * lane; j < D; j += 256) {
            const float4 t = *reinterpret_cast<const float4*>(ar + j), x = *reinterpret_cast<const float4*>(xr + j);
            float4 o;
            o.x = elem(t.x, x.x, ll); o.y = elem(t.y, x.y, ll); o.z = elem(t.z, x.z, ll); o.w = elem(t.w, x.w, ll);
            *reinterpret_cast<float4*>(ar + j) = o;
        }
    } else {
        for (int j = lane; j < D; j += 64) ar[j] = elem(ar[j], xr[j], ll);
    }
    ll = wave_sum(ll);
    xx = wave_sum(xx);
    if (lane == 0) {
        px_loss[i] = (mask && mask[i] == 0) ? 0.f : sc * (lat[i] - ll);
        x2[i] = xx;
    }
}

// joint L2 norm of every example's gradient by the outer-product identity, clip factor c_i (0 for masked rows); the rows of
// the delta arrays are staged in LDS while their squares are summed and written back scaled by c_i (svi.py:121-122
// folded into the sums), so the deltas are read once and written once (a separate rescaling pass read them a second time).
// One term per dense layer, in the order decoder output layer .. decoder first layer, latent heads, encoder last .. first:
// ||grad||^2 = sum_t (|input_t|^2 + 1) (|delta_t|^2 [+ |delta'_t|^2])  (the + 1 is the bias; the heads share their input)
#define D3P_VAE_MAX_TERMS 6
struct NormTerm {
    const float* in;  // B x in_n, row stride in_ld; nullptr: |x_i|^2 comes from x2 (left by k_vae_out)
    float* d0;        // B x d_n, row stride d_ld: the layer's delta, rescaled in place
    float* d1;        // the second head's delta (same shape), or nullptr
    int in_ld, in_n, d_ld, d_n;
};
struct NormArgs {
    NormTerm t[D3P_VAE_MAX_TERMS];
    int n_terms;
    int stage;  // floats of LDS per wave = sum of the delta widths
    const float* x2;
    const uint8_t* mask;
    uint32_t B;
    float clip;
    float* cf;
    float* norms;  // nullable
    int scale_back;        // 0: the deltas stay as they are -- the weight-gradient products apply cf themselves (GemmArgs::b_row_scale)
    float* px_loss;        // the LAST workgroup of the launch sums px_loss and counts the unmasked examples into loss_n[0..1]
    float* loss_n;         // (fixed order; was a launch of its own)
    // the output layer's epilogue left per-group partial sums instead of px_loss / x2 (GemmArgs::epi 4): every row's wave finishes
    // them here (vae_out_finish_row) -- px_loss is then complete only when this launch ends, so the last workgroup leaves loss_n[0]
    // alone and a later launch sums px_loss (k_vae_finalize / k_vae_tile_sums: vae_block_sum)
    const float* ep_ll;    // nullable: [ep_groups][B]
    const float* ep_xx;
    const float* lat;
    int ep_groups;         // <= 64
    float ep_sc;
};

// (the finishing step of GemmArgs::epi 4 for one example: px_loss[i] = sc (lat_i - sum_g ll[g][i]) mask_i; returns |x_i|^2)
__device__ __forceinline__ float vae_out_finish_row(const float* __restrict__ ep_ll, const float* __restrict__ ep_xx, int groups, uint32_t B,
                                                    uint32_t i, int lane, const float* __restrict__ lat, float sc, bool live,
                                                    float* __restrict__ px_loss)
{
    float l = 0.f, x = 0.f, sl, sx;
    if (lane < groups) {
        l = ep_ll[(size_t)lane * B + i];
        x = ep_xx[(size_t)lane * B + i];
    }
    wave_sum2(l, x, sl, sx);
    if (lane == 0) px_loss[i] = live ? sc * (lat[i] - sl) : 0.f;
    return sx;
}

// sum of v[0 .. n - 1] by one workgroup of 256 threads, fixed order; lds: 256 floats; every thread gets the total
__device__ __forceinline__ float vae_block_sum(const float* __restrict__ v, uint32_t n, float* lds)
{
    float s = 0.f;
    for (uint32_t i = threadIdx.x; i < n; i += 256) s += v[i];
    lds[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) lds[threadIdx.x] += lds[threadIdx.x + off];
        __syncthreads();
    }
    const float tot = lds[0];
    __syncthreads();
    return tot;
}

// this lane's share of a row's sum of squares (16-byte loads: elements 4 l .. 4 l + 3, + 256, ...; rows that cannot take them:
// elements l, l + 64, ...), copying what it reads to `keep` when given -- the wave sums come later, all terms at once
__device__ __forceinline__ bool row_vec4(const float* r, int n) { return (n & 3) == 0 && (reinterpret_cast<uintptr_t>(r) & 15u) == 0; }
__device__ __forceinline__ float row_sumsq_lane(const float* __restrict__ r, int n, int lane, float* __restrict__ keep)
{
    float s = 0.f;
    if (row_vec4(r, n)) {
        for (int j = 4 * lane; j < n; j += 256) {
            const float4 v = *reinterpret_cast<const float4*>(r + j);
            if (keep) *reinterpret_cast<float4*>(keep + j) = v;
            s = __fmaf_rn(v.x, v.x, s); s = __fmaf_rn(v.y, v.y, s); s = __fmaf_rn(v.z, v.z, s); s = __fmaf_rn(v.w, v.w, s);
        }
    } else {
        for (int j = lane; j < n; j += 64) {
            const float v = r[j];
            if (keep) keep[j] = v;
            s = __fmaf_rn(v, v, s);
        }
    }
    return s;
}
__device__ __forceinline__ void row_scale_back(float* __restrict__ r, int n, int lane, const float* __restrict__ keep, float c)
{
    if (row_vec4(r, n)) {
        for (int j = 4 * lane; j < n; j += 256) {
            const float4 v = *reinterpret_cast<const float4*>(keep + j);
            *reinterpret_cast<float4*>(r + j) = make_float4(v.x * c, v.y * c, v.z * c, v.w * c);
        }
    } else {
        for (int j = lane; j < n; j += 64) r[j] = keep[j] * c;
    }
}

__global__ void k_vae_norms(NormArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float norm_stage[];  // 4 waves x a.stage
    if (blockIdx.x == gridDim.x - 1) {  // sums[P] = sum_i px_loss[i], sums[P + 1] = number of unmasked examples
        float* l = norm_stage;
        float* c = norm_stage + 256;
        float s = 0.f, n = 0.f;
        for (uint32_t i = threadIdx.x; i < a.B; i += 256) {
            s += a.px_loss[i];
            n += (a.mask && a.mask[i] == 0) ? 0.f : 1.f;
        }
        l[threadIdx.x] = s;
        c[threadIdx.x] = n;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) { l[threadIdx.x] += l[threadIdx.x + off]; c[threadIdx.x] += c[threadIdx.x + off]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (!a.ep_ll) a.loss_n[0] = l[0];   // (fused output layer: px_loss is being written by this very launch)
            a.loss_n[1] = c[0];
        }
        return;
    }
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= a.B) return;
    float* keep = norm_stage + (size_t)(threadIdx.x >> 6) * a.stage;
    const float x2_row = a.ep_ll ? vae_out_finish_row(a.ep_ll, a.ep_xx, a.ep_groups, a.B, i, lane, a.lat, a.ep_sc, !(a.mask && a.mask[i] == 0), a.px_loss)
                                 : a.x2[i];
    // every term's loads first (per-lane partial sums: nothing waits for a wave sum between two terms), then all wave sums
    float pin[D3P_VAE_MAX_TERMS], pd[D3P_VAE_MAX_TERMS];
    {
        float* k = keep;
#pragma unroll
        for (int t = 0; t < D3P_VAE_MAX_TERMS; ++t) {
            pin[t] = pd[t] = 0.f;
            if (t < a.n_terms) {
                const NormTerm& q = a.t[t];
                if (q.in) pin[t] = row_sumsq_lane(q.in + (size_t)i * q.in_ld, q.in_n, lane, nullptr);
                pd[t] = row_sumsq_lane(q.d0 + (size_t)i * q.d_ld, q.d_n, lane, a.scale_back ? k : nullptr);
                k += (q.d_n + 3) & ~3;
                if (q.d1) {
                    pd[t] += row_sumsq_lane(q.d1 + (size_t)i * q.d_ld, q.d_n, lane, a.scale_back ? k : nullptr);
                    k += (q.d_n + 3) & ~3;
                }
            }
        }
    }
    float n2 = 0.f;
#pragma unroll
    for (int t = 0; t < D3P_VAE_MAX_TERMS; ++t) {
        if (t < a.n_terms) {
            float in2, d;
            wave_sum2(pin[t], pd[t], in2, d);
            if (!a.t[t].in) in2 = x2_row;
            n2 += (in2 + 1.0f) * d;
        }
    }
    const float nrm = sqrtf(n2);
    const bool live = !(a.mask && a.mask[i] == 0);
    const float c = live ? 1.0f / fmaxf(1.0f, nrm / a.clip) : 0.f;  // svi.py:121-122; masked rows contribute nothing
    if (lane == 0) {
        a.cf[i] = c;
        if (a.norms) a.norms[i] = live ? nrm : 0.f;
    }
    if (!a.scale_back) return;
    // every lane reads back exactly the LDS words it wrote: no barrier needed
    float* k = keep;
    for (int t = 0; t < a.n_terms; ++t) {
        const NormTerm& q = a.t[t];
        row_scale_back(q.d0 + (size_t)i * q.d_ld, q.d_n, lane, k, c);
        k += (q.d_n + 3) & ~3;
        if (q.d1) {
            row_scale_back(q.d1 + (size_t)i * q.d_ld, q.d_n, lane, k, c);
            k += (q.d_n + 3) & ~3;
        }
    }
}

// sums[P] = sum_i px_loss[i], sums[P + 1] = number of unmasked examples (one workgroup, fixed order)
__global__ void __launch_bounds__(256) k_vae_loss_n(const float* __restrict__ px_loss, const uint8_t* __restrict__ mask, uint32_t B,
                                                    float* __restrict__ out)
{
    __shared__ float l[256], c[256];
    float s = 0.f, n = 0.f;
    for (uint32_t i = threadIdx.x; i < B; i += 256) {
        s += px_loss[i];
        n += (mask && mask[i] == 0) ? 0.f : 1.f;
    }
    l[threadIdx.x] = s;
    c[threadIdx.x] = n;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { l[threadIdx.x] += l[threadIdx.x + off]; c[threadIdx.x] += c[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = l[0]; out[1] = c[0]; }
}

// the finishing step of GemmArgs::epi 4 as a launch of its own, where no norm kernel follows the forward pass (evaluate)
__global__ void __launch_bounds__(256) k_vae_out_finish(const float* __restrict__ ep_ll, const float* __restrict__ ep_xx, int groups, uint32_t B,
                                                        const float* __restrict__ lat, float sc, const uint8_t* __restrict__ mask,
                                                        float* __restrict__ px_loss, float* __restrict__ x2)
{
    const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= B) return;
    const float xx = vae_out_finish_row(ep_ll, ep_xx, groups, B, i, lane, lat, sc, !(mask && mask[i] == 0), px_loss);
    if (lane == 0) x2[i] = xx;
}

// mean, Gaussian mechanism, rescale (svi.py:343-346, :365-375), numpyro Adam (svi.py:379-393) over the P parameters
#define D3P_VAE_MAX_BLOCKS 7  // [W | b] blocks of the flat layout: 2 nh + 3 with nh <= 2 hidden layers

// weight-gradient blocks whose split-K partial tiles were left unreduced: block b = columns [w_off[b], w_off[b + 1]) of the flat
// layout, w_splits[b] tiles (0: the product wrote its sums itself)
struct VaeTiles {
    const float* wpart;                                         // nullptr: no block has tiles
    uint32_t w_off[D3P_VAE_MAX_BLOCKS + 1];                     // first column of block b (unused entries = P)
    uint32_t w_base[D3P_VAE_MAX_BLOCKS], w_tile[D3P_VAE_MAX_BLOCKS], w_ld[D3P_VAE_MAX_BLOCKS], w_coff[D3P_VAE_MAX_BLOCKS],
        w_out[D3P_VAE_MAX_BLOCKS];                              // its tiles: wpart + w_base, w_tile apart, element (r, c) of the
    int w_splits[D3P_VAE_MAX_BLOCKS];                           // block at r * w_ld + w_coff + c, c < w_out
};

// column col's sum over its block's tiles, in fixed order (`direct` = what the product wrote when the block has none)
__device__ __forceinline__ float vae_tile_sum(const VaeTiles& a, size_t col, float direct)
{
    if (!a.wpart) return direct;
    int b = 0;
#pragma unroll
    for (int k = 1; k < D3P_VAE_MAX_BLOCKS; ++k) b += (col >= a.w_off[k]) ? 1 : 0;
    if (a.w_splits[b] <= 0) return direct;
    const uint32_t e = (uint32_t)col - a.w_off[b];
    const float* t = a.wpart + a.w_base[b] + (size_t)(e / a.w_out[b]) * a.w_ld[b] + a.w_coff[b] + e % a.w_out[b];
    // (all tiles requested at once -- a loop over a run-time count is one memory round trip per tile: 16.6 -> 13.4 us)
    const int nz = a.w_splits[b];
    const size_t tile = a.w_tile[b];
    float tv[D3P_WPART_SPLITS];
#pragma unroll
    for (int z = 0; z < D3P_WPART_SPLITS; ++z) tv[z] = z < nz ? t[(size_t)z * tile] : 0.f;
    float tot = 0.f;
#pragma unroll
    for (int z = 0; z < D3P_WPART_SPLITS; ++z) tot += z < nz ? tv[z] : 0.f;
    return tot;
}

// sums[col] := the tile sums (stage API and data-parallel local sums: the sums leave the device function as one vector)
// px_loss != nullptr (fused output layer): sums[P] = sum_i px_loss[i] too (workgroup 0; the norm kernel could not: see NormArgs)
// col0 .. col1 - 1: the columns of this launch (a bucket of the data-parallel step's reduce: VaeBuckets)
__global__ void __launch_bounds__(256) k_vae_tile_sums(VaeTiles a, float* __restrict__ sums, size_t P, const float* __restrict__ px_loss, uint32_t B,
                                                       size_t col0, size_t col1)
{
    __shared__ float lds[256];
    if (px_loss && blockIdx.x == 0) {
        const float tot = vae_block_sum(px_loss, B, lds);
        if (threadIdx.x == 0) sums[P] = tot;
    }
    const size_t col = col0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col < col1) sums[col] = vae_tile_sum(a, col, sums[col]);
}

struct VaeFinalArgs {
    const float* sums;  // P + 2
    VaeTiles tiles;     // (single-device update: k_vae_finalize sums the tiles itself)
    const float* noise;
    const float* in_params;  // state before the update (== params / adam_m / adam_v, or the old state's arrays when the update
    const float* in_m;       // is out of place: DPSVI.update returns a NEW state, svi.py:395-434)
    const float* in_v;
    float* params;
    float* adam_m;
    float* adam_v;
    const int32_t* step;
    float* loss_out;
    float* grad_out;
    size_t P;
    uint32_t B;
    d3p_dpsvi_hyper h;
    float obs_scale;
    const float* px_loss;   // nullable (fused output layer, single-device update): the loss sum is taken here, sum_i px_loss[i] over
    uint32_t B_local;       // B_local examples, instead of from sums[P] (NormArgs)
};

// one parameter column of the update: mean + noise (svi.py:343-346, :365-375), rescale, numpyro Adam (svi.py:379-393)
__device__ __forceinline__ void vae_finalize_col(const VaeFinalArgs& a, size_t col, float tot, float n, float factor, float bc0, float bc1)
{
    const float Bf = (float)a.B;
    const float g = (tot / Bf + a.noise[col] * (a.h.dp_scale * (a.h.clip / n))) * a.obs_scale * factor;
    if (a.grad_out) a.grad_out[col] = g;
    float m = a.in_m[col], v = a.in_v[col];
    m = (1.0f - a.h.b1) * g + a.h.b1 * m;
    v = (1.0f - a.h.b2) * g * g + a.h.b2 * v;
    const float mhat = m / bc0;
    const float vhat = v / bc1;
    a.params[col] = a.in_params[col] - a.h.lr * mhat / (sqrtf(vhat) + a.h.adam_eps);
    a.adam_m[col] = m;
    a.adam_v[col] = v;
}

__global__ void __launch_bounds__(256) k_vae_finalize(VaeFinalArgs a)
{
    __shared__ float bc[2];  // Adam's bias corrections 1 - b^(i + 1): two powf per workgroup instead of per column
    __shared__ float lsum[256];
    if (threadIdx.x < 2) bc[threadIdx.x] = 1.0f - powf(threadIdx.x ? a.h.b2 : a.h.b1, (float)(*a.step + 1));
    __syncthreads();
    const size_t col = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float n = a.sums[a.P + 1], Bf = (float)a.B;
    const float factor = (n == 0.f) ? 0.f : Bf / n;
    if (blockIdx.x == 0 && a.loss_out) {   // (workgroup-uniform)
        const float ls = a.px_loss ? vae_block_sum(a.px_loss, a.B_local, lsum) : a.sums[a.P];
        if (threadIdx.x == 0) *a.loss_out = (ls / Bf) * a.obs_scale * factor;
    }
    if (col >= a.P) return;
    vae_finalize_col(a, col, vae_tile_sum(a.tiles, col, a.sums[col]), n, factor, bc[0], bc[1]);
}

// The data-parallel step's tile sums, full-mesh all-reduce (d3p_fmesh.hip: reduce-scatter, rank-order owner sums, all-gather as tagged
// 8-byte words through the peers' hipIpc-mapped inboxes) and update in ONE launch: the scatter phase takes a column's value straight
// from the split-K partial tiles (k_vae_tile_sums' work), the gather phase applies noise + Adam to a column the moment its sum over the
// ranks has arrived (k_vae_finalize's work) -- two launches and two passes over the 2.76 MB of sums less per step.  The owner stores
// its chunk's sums into its OWN gather slots too, so that every column (and the global example count every column's update needs) is
// read the same way.  Same arithmetic, column by column, as tile sums -> d3p_fmesh_allreduce -> k_vae_finalize: bit for bit.
__global__ void __launch_bounds__(256) k_vae_fmesh_step(FMeshArgs m, VaeFinalArgs f)
{
    constexpr int U = 4;
    __shared__ float bc[2];
    if (threadIdx.x < 2) bc[threadIdx.x] = 1.0f - powf(threadIdx.x ? f.h.b2 : f.h.b1, (float)(*f.step + 1));
    __syncthreads();
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (uint64_t)gridDim.x * blockDim.x;
    char* const mine = m.peer[m.rank];
    const size_t sc_par = (size_t)m.parity * m.world * m.chunk;
    auto local = [&](uint64_t i) { return i < (uint64_t)f.P ? vae_tile_sum(f.tiles, (size_t)i, f.sums[i]) : f.sums[i]; };   // [P]: loss sum, [P + 1]: count
    // ---- reduce-scatter
    for (uint64_t i0 = tid; i0 < m.n; i0 += U * nthreads) {
        float v[U];
        int o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t i = i0 + (uint64_t)u * nthreads;
            o[u] = i < m.n ? (int)(i / m.chunk) : m.rank;
            v[u] = o[u] != m.rank ? local(i) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t i = i0 + (uint64_t)u * nthreads;
            if (o[u] != m.rank) fm_store(m.peer[o[u]], sc_par + (size_t)m.rank * m.chunk + (i - (uint64_t)o[u] * m.chunk), v[u], m.tag);
        }
    }
    // ---- owner sums of my chunk in rank order; the sums go to EVERY rank's gather slot [parity][my rank], mine included
    const uint64_t lo = (uint64_t)m.rank * m.chunk, hi = lo + m.chunk < m.n ? lo + m.chunk : m.n;
    bool ok = true;
    for (uint64_t i = lo + tid; i < hi && ok; i += nthreads) {
        const uint64_t j = i - lo;
        const float own = local(i);
        unsigned long long w[D3P_FMESH_MAX_WORLD];
        bool all = m.world == 1;
        for (uint32_t spins = 0; spins < D3P_FMESH_WAIT_ROUNDS && !all; ++spins) {
#pragma unroll
            for (int r = 0; r < D3P_FMESH_MAX_WORLD; ++r)
                if (r < m.world && r != m.rank)
                    w[r] = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(mine) + sc_par + (size_t)r * m.chunk + j, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_SYSTEM);
            all = true;
#pragma unroll
            for (int r = 0; r < D3P_FMESH_MAX_WORLD; ++r)
                if (r < m.world && r != m.rank) all = all && (uint32_t)(w[r] >> 32) == m.tag;
            if (!all && (spins & 255u) == 255u && __hip_atomic_load(m.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
        }
        if (!all) { ok = false; break; }
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < D3P_FMESH_MAX_WORLD; ++r)
            if (r < m.world) {
                const float v = r == m.rank ? own : __uint_as_float((uint32_t)w[r]);
                s = r == 0 ? v : s + v;
            }
        for (int p = 0; p < m.world; ++p) fm_store(m.peer[p] + m.gather_off, sc_par + (size_t)m.rank * m.chunk + j, s, m.tag);
    }
    // ---- gather + update: the example count first (every column's update needs it), then U columns' sums requested together
    const unsigned long long* const gin = reinterpret_cast<const unsigned long long*>(mine + m.gather_off) + sc_par;
    auto gword = [&](uint64_t i) { const uint64_t o = i / m.chunk; return (size_t)o * m.chunk + (size_t)(i - o * m.chunk); };
    float n = 0.f;
    {
        const size_t wn = gword((uint64_t)f.P + 1u);
        bool have = false;
        for (uint32_t spins = 0; spins < D3P_FMESH_WAIT_ROUNDS && ok; ++spins) {
            const unsigned long long w = __hip_atomic_load(gin + wn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((uint32_t)(w >> 32) == m.tag) { n = __uint_as_float((uint32_t)w); have = true; break; }
            if ((spins & 255u) == 255u && __hip_atomic_load(m.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
        }
        ok = ok && have;
    }
    const float Bf = (float)f.B, factor = (n == 0.f) ? 0.f : Bf / n;
    for (uint64_t i0 = tid; i0 < m.n && ok; i0 += U * nthreads) {
        size_t word[U];
        bool need[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t i = i0 + (uint64_t)u * nthreads;
            need[u] = i <= (uint64_t)f.P;   // the P columns and the loss sum
            word[u] = need[u] ? gword(i) : 0;
        }
        unsigned long long w[U];
        bool all = false;
        for (uint32_t spins = 0; spins < D3P_FMESH_WAIT_ROUNDS && !all; ++spins) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (need[u]) w[u] = __hip_atomic_load(gin + word[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            all = true;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (need[u]) all = all && (uint32_t)(w[u] >> 32) == m.tag;
            if (!all && (spins & 255u) == 255u && __hip_atomic_load(m.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
        }
        if (!all) { ok = false; break; }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!need[u]) continue;
            const uint64_t i = i0 + (uint64_t)u * nthreads;
            const float s = __uint_as_float((uint32_t)w[u]);
            if (i < (uint64_t)f.P) vae_finalize_col(f, (size_t)i, s, n, factor, bc[0], bc[1]);
            else if (f.loss_out) *f.loss_out = (s / Bf) * f.obs_scale * factor;
        }
    }
    if (!ok) {
        uint32_t expect = 0u;
        (void)__hip_atomic_compare_exchange_strong(m.status, &expect, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// rows of the five delta arrays scaled by the clip factors in one launch
// All keys of one update in ONE launch (they were three launches + a step-counter launch + a 64-byte copy, ~5 us each):
// keys[0..47] = [next | gradient | perturbation] = split(state_key, 3) (svi.py:208-211), keys[48 ..] =
// split(perturbation_key, n_sites) (svi.py:491; n_sites = 10 or 14 leaves), keys[D3P_VAE_KEY_JAX ..+1] =
// convert_to_jax_rng_key(gradient_key).  advance: also write the next state key into the other key slot, save the optimiser
// step index in keys[D3P_VAE_KEY_STEP] for k_vae_finalize and advance it.
#define D3P_VAE_KEY_JAX (48 + 16 * D3P_VAE_MAX_LEAVES)
#define D3P_VAE_KEY_STEP (D3P_VAE_KEY_JAX + 2)
#define D3P_VAE_KEY_WORDS (D3P_VAE_KEY_JAX + 4)
// Further workgroups of the launch do work of the step that depends on nothing but its inputs (a launch of their own cost as
// much as this one): workgroups 1 .. x_blocks the exactness pass over the batch (exact16_pass); the ones behind them pack the two
// latent heads, which lie H Z + Z apart in the flat layout with rows of Z floats (no 16-byte fetches: the head products took the
// scalar 64 x 64 kernel), side by side into wcat (HE x 2 Z = [Wl | Ws]) and transposed into wcatT (2 Z x HE = [Wl^T ; Ws^T]).
struct KeysExtra {
    const float* x;
    size_t x_n4;
    uint32_t* x_flag;
    uint32_t x_nonce;
    unsigned x_blocks;
    const float *wl, *wsd;   // the heads' weights (HE x Z each)
    float *wcat, *wcatT;
    int HE, Z;
    unsigned pack_blocks;
    // the run loop's step (d3p_dpvi_vae_run): the workgroups behind the packing ones make the step's batch indices --
    // fold_in(batch_key, batch_i) (minibatch.py:230), its 30 round constants, the Feistel permutation of positions 0 .. n_idx - 1
    // (util.py:248-301), every workgroup deriving the constants for itself (two dependent quad-lane ChaCha blocks) like k_sampler
    const uint32_t* batch_key;   // nullable
    uint32_t batch_i, capacity, n_idx;
    int bits_lower, bits_upper;
    uint32_t* idx;
};

__global__ void __launch_bounds__(256) k_vae_keys(const uint32_t* __restrict__ cur_key, uint32_t* __restrict__ keys,
                                                  uint32_t* __restrict__ next_slot, const int32_t* __restrict__ step,
                                                  int32_t* __restrict__ step_out, int advance, int n_sites, KeysExtra ex)
{
    if (blockIdx.x > ex.x_blocks + ex.pack_blocks) {
        __shared__ uint32_t f_key[16], f_rc[32];
        const int tid = threadIdx.x, quad = tid >> 2, q = tid & 3;
        if (quad == 0) {
            uint32_t ka, kb;
            derive_child_quad(ex.batch_key, 0u, D3P_TAG_FOLD, ex.batch_i, ka, kb);
            f_key[q] = ex.batch_key[q];
            f_key[4 + q] = ka;
            f_key[8 + q] = kb;
            f_key[12 + q] = 0u;
        }
        __syncthreads();
        if (quad < 2) {  // round constants: keystream blocks 0, 1 (util.py:240-246), column 0 forced odd
            uint32_t w[4];
            keystream_block_quad(f_key, (uint32_t)quad, w[0], w[1], w[2], w[3]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int g = 16 * quad + 4 * i + q;
                if (g < 30) f_rc[g] = (g % 3 == 0) ? (w[i] | 1u) : w[i];
            }
        }
        __syncthreads();
        const uint32_t p = (blockIdx.x - ex.x_blocks - ex.pack_blocks - 1) * blockDim.x + (uint32_t)tid;
        if (p < ex.n_idx) ex.idx[p] = feistel_permute_dev(f_rc, ex.capacity, ex.bits_lower, ex.bits_upper, p);
        return;
    }
    if (blockIdx.x > ex.x_blocks) {
        const unsigned t = (blockIdx.x - ex.x_blocks - 1) * blockDim.x + threadIdx.x;
        const unsigned Z2 = 2u * ex.Z;
        if (t < (unsigned)ex.HE * Z2) {
            const unsigned k = t / Z2, n = t % Z2;
            const float v = n < (unsigned)ex.Z ? ex.wl[k * ex.Z + n] : ex.wsd[k * ex.Z + n - ex.Z];
            ex.wcat[t] = v;
            ex.wcatT[(size_t)n * ex.HE + k] = v;
        }
        return;
    }
    if (blockIdx.x > 0) {
        exact16_pass(ex.x, ex.x_n4, ex.x_flag, ex.x_nonce, blockIdx.x - 1, ex.x_blocks);
        return;
    }
    // one quad of lanes per derivation (4-lane ChaCha block, d3p_device.h), on the first wave: the launch is pure latency
    __shared__ uint32_t sk[3][16];
    const bool kt = threadIdx.x < 64;
    const int lane = threadIdx.x & 63, quad = lane >> 2, q = lane & 3;
    auto store_child = [&](uint32_t* dst, const uint32_t* parent, uint32_t a, uint32_t b) {
        dst[q] = parent[q];
        dst[4 + q] = a;
        dst[8 + q] = b;
        dst[12 + q] = 0u;
    };
    if (kt) {
        uint32_t a, b;
        derive_child_quad(cur_key, quad < 3 ? (uint32_t)quad : 0u, D3P_TAG_SPLIT, 0u, a, b);
        if (quad < 3) {
            store_child(keys + 16 * quad, cur_key, a, b);
            store_child(sk[quad], cur_key, a, b);
            if (quad == 0 && advance) store_child(next_slot, cur_key, a, b);
        }
        if (lane == 63 && advance) {
            const int32_t i = *step;
            keys[D3P_VAE_KEY_STEP] = (uint32_t)i;
            *step_out = i + 1;  // (step_out == step, or the new state's counter when the update is out of place)
        }
    }
    __syncthreads();
    if (kt) {
        // quad 0: block 0 of the gradient key's stream -> jax key; quads 1..n_sites (<= 15): split(perturbation_key, n_sites)
        const uint32_t* parent = quad == 0 ? sk[1] : sk[2];
        const bool site = quad >= 1 && quad <= n_sites;
        uint32_t a, b;
        derive_child_quad(parent, site ? (uint32_t)(quad - 1) : 0u, quad == 0 ? 0u : D3P_TAG_SPLIT, 0u, a, b);
        if (quad == 0 && q < 2) keys[D3P_VAE_KEY_JAX + q] = a;
        if (site) store_child(keys + 48 + 16 * (quad - 1), parent, a, b);
    }
}

// The network as lists of dense layers.  Hidden widths hs[0 .. nh - 1]: [H] (the reference, examples/vae.py:80-85) or
// [H, H2] (BASELINE config 5's 784 -> [400, 200] variant, model->H2 > 0):
//   encoder (guide)  x -> hs[0] -> .. -> hs[nh - 1] : dense layers enc[0 .. nh - 1] (softplus), then the heads (Wl, bl), (Ws, bs)
//   decoder (model)  z -> hs[nh - 1] -> .. -> hs[0] -> D : dense layers dec[0 .. nh] (softplus after all but the last)
// Flat layout = tree_flatten order of {'decoder$params', 'encoder$params'}: decoder layers, encoder layers, Wl, bl, Ws, bs; a
// layer is [W (in x out) | b (out)] (stax.Dense).  nh = 1: V1, c1, V2, c2, W1, b1, Wl, bl, Ws, bs -- 10 leaves, 5 blocks.
struct VaeDense { size_t W, b; int in, out; };
struct VaeNet {
    int nh, D, Z, HE;  // HE = hs[nh - 1]: width of the encoder's last hidden layer = input of the heads
    VaeDense dec[3], enc[2];
    size_t Wl, bl, Ws, bs, P;
    int n_leaves() const { return 2 * (2 * nh + 1) + 4; }
    int n_blocks() const { return 2 * nh + 3; }
    // [W | b] block b of the flat layout: decoder layers, encoder layers, Wl, Ws
    const VaeDense* block_layer(int blk) const { return blk <= nh ? &dec[blk] : blk <= 2 * nh ? &enc[blk - nh - 1] : nullptr; }
};

static VaeNet vae_net(const d3p_vae_model* m)
{
    VaeNet n;
    memset(&n, 0, sizeof(n));
    n.nh = m->H2 > 0 ? 2 : 1;
    n.D = m->D;
    n.Z = m->Z;
    const int hs[2] = {m->H, m->H2};
    n.HE = hs[n.nh - 1];
    size_t off = 0;
    auto dense = [&](VaeDense* l, int in, int out) {
        l->in = in; l->out = out;
        l->W = off; off += (size_t)in * out;
        l->b = off; off += (size_t)out;
    };
    for (int l = 0; l <= n.nh; ++l) dense(&n.dec[l], l == 0 ? n.Z : hs[n.nh - l], l == n.nh ? n.D : hs[n.nh - l - 1]);
    for (int l = 0; l < n.nh; ++l) dense(&n.enc[l], l == 0 ? n.D : hs[l - 1], hs[l]);
    n.Wl = off; off += (size_t)n.HE * n.Z;
    n.bl = off; off += (size_t)n.Z;
    n.Ws = off; off += (size_t)n.HE * n.Z;
    n.bs = off; off += (size_t)n.Z;
    n.P = off;
    return n;
}

struct VaeWorkspace {
    float *he[2], *sge[2];   // encoder hidden activations and sigmoid(pre-activation) = softplus'
    float *hd[2], *sgd[2];   // decoder hidden, likewise (hd[l] = output of dec[l])
    float *dd[2], *de[2];    // deltas at the pre-activations of dec[l] / enc[l]
    float *zl, *u, *eps, *a, *dz, *du;
    float *lat, *px_loss, *x2, *cf, *sums, *noise, *part, *wpart;
    size_t part_floats;
    uint32_t* keys;  // 3 x 16 split + up to 14 x 16 site keys + jax key + step index (D3P_VAE_KEY_*)
    uint32_t* x_exact16;  // one word: the batch X is exactly bf16 (GemmArgs::a_exact16), set per forward pass
    float *wcat, *wcatT;  // the latent heads packed for the step (k_vae_keys): [Wl | Ws] (HE x 2 Z) and its transpose
    float *ep_ll, *ep_xx; // per-group partial row sums of the output layer's epilogue (GemmArgs::epi 4): [ceil(D / 32)][B] each
};

// one step of the native run loop (d3p_dpvi_vae_run): the batch is rows of a resident table, chosen by the Feistel sampler
struct VaeRunStep {
    const uint32_t* batch_key;   // batchifier state (device)
    uint32_t batch_i;            // fold_in data: index of the batch (minibatch.py:230)
    const float* table;          // n_rows x D
    uint32_t n_rows;
    uint32_t* idx;               // B indices (written)
};

// what the key launch of an update has already done for the passes that follow it (vae_step_keys)
struct VaeStepPrep {
    bool x_checked = false;     // the exactness pass over X of THIS forward pass has been enqueued
    bool heads_packed = false;  // ws.wcat / ws.wcatT hold the heads of the parameters the pass runs on
};

static size_t vae_carve(const d3p_vae_model* m, uint32_t B, char* base, VaeWorkspace* ws)
{
    const VaeNet N = vae_net(m);
    const size_t D = (size_t)N.D, Z = (size_t)N.Z, P = N.P;
    size_t off = 0;
    auto take = [&](size_t n_floats) { size_t o = off; off += align_up_v(n_floats * sizeof(float), 256); return base ? (float*)(base + o) : nullptr; };
    float* q;
    if (ws) memset(ws, 0, sizeof(*ws));
    for (int l = 0; l < N.nh; ++l) {
        q = take(B * (size_t)N.enc[l].out); if (ws) ws->he[l] = q;
        q = take(B * (size_t)N.enc[l].out); if (ws) ws->sge[l] = q;
    }
    q = take(B * 2 * Z); if (ws) { ws->zl = q; ws->u = q + Z; }    // [z_loc -> z | log z_std -> z_std]: B x 2 Z, row stride 2 Z
    q = take(B * Z); if (ws) ws->eps = q;
    for (int l = 0; l < N.nh; ++l) {
        q = take(B * (size_t)N.dec[l].out); if (ws) ws->hd[l] = q;
        q = take(B * (size_t)N.dec[l].out); if (ws) ws->sgd[l] = q;
    }
    q = take(B * D); if (ws) ws->a = q;
    for (int l = 0; l < N.nh; ++l) { q = take(B * (size_t)N.dec[l].out); if (ws) ws->dd[l] = q; }
    q = take(B * 2 * Z); if (ws) { ws->dz = q; ws->du = q + Z; }  // [dz | du], likewise
    for (int l = 0; l < N.nh; ++l) { q = take(B * (size_t)N.enc[l].out); if (ws) ws->de[l] = q; }
    q = take(B); if (ws) ws->lat = q;
    q = take(B); if (ws) ws->px_loss = q;
    q = take(B); if (ws) ws->x2 = q;
    q = take(B); if (ws) ws->cf = q;
    q = take(P + 2); if (ws) ws->sums = q;
    q = take(P); if (ws) ws->noise = q;
    q = take(D3P_VAE_KEY_WORDS); if (ws) ws->keys = (uint32_t*)q;
    const size_t pf = 16 * (D + 1) * (size_t)m->H;  // split-K partial tiles: up to 16 splits of the largest weight matrix
    q = take(pf); if (ws) { ws->part = q; ws->part_floats = pf; }
    q = take((size_t)D3P_WPART_SPLITS * P); if (ws) ws->wpart = q;  // unreduced weight-gradient tiles
    q = take(64); if (ws) ws->x_exact16 = (uint32_t*)q;
    q = take((size_t)N.HE * 2 * Z); if (ws) ws->wcat = q;
    q = take((size_t)N.HE * 2 * Z); if (ws) ws->wcatT = q;
    q = take((size_t)cdiv(D, 32) * B); if (ws) ws->ep_ll = q;
    q = take((size_t)cdiv(D, 32) * B); if (ws) ws->ep_xx = q;
    return off;
}

static int vae_validate(const d3p_vae_model* m, const char* what)
{
    if (!m) return fail(D3P_E_INVALID_ARG, "%s: null model", what);
    if (!(m->D >= 1 && m->H >= 1 && m->Z >= 1 && m->H2 >= 0 && m->scale > 0.f && m->inv_obs > 0.f))
        return fail(D3P_E_INVALID_ARG, "%s: bad model (D, H, Z >= 1, H2 >= 0, scale > 0, inv_obs > 0)", what);
    return D3P_OK;
}

// [W | b] blocks of the flat layout and their unreduced tiles in ws.wpart: the dense layers, then Wl and Ws -- which come from ONE
// product with N = 2 Z: shared tiles of (HE + 1) x 2 Z in the region of the Wl block
static VaeTiles vae_tiles(const VaeNet& N, const VaeWorkspace& ws, const int* w_splits)
{
    VaeTiles f;
    memset(&f, 0, sizeof(f));
    f.wpart = w_splits ? ws.wpart : nullptr;
    const int nh = N.nh, n_blocks = N.n_blocks();
    for (int b = 0; b < n_blocks; ++b) {
        const VaeDense* lay = N.block_layer(b);
        const size_t first = lay ? lay->W : (b == 2 * nh + 1 ? N.Wl : N.Ws);
        const size_t next = b + 1 < n_blocks ? (N.block_layer(b + 1) ? N.block_layer(b + 1)->W : (b + 1 == 2 * nh + 1 ? N.Wl : N.Ws)) : N.P;
        f.w_off[b] = (uint32_t)first;
        f.w_base[b] = (uint32_t)(D3P_WPART_SPLITS * first);
        f.w_tile[b] = (uint32_t)(next - first);
        f.w_ld[b] = f.w_out[b] = (uint32_t)(lay ? lay->out : N.Z);
        f.w_coff[b] = 0;
        f.w_splits[b] = w_splits ? w_splits[b] : 0;
    }
    const int bl = 2 * nh + 1, bs = 2 * nh + 2;
    f.w_tile[bl] = f.w_tile[bs] = f.w_tile[bl] + f.w_tile[bs];
    f.w_ld[bl] = f.w_ld[bs] = 2u * (uint32_t)N.Z;
    f.w_base[bs] = f.w_base[bl];
    f.w_coff[bs] = (uint32_t)N.Z;
    for (int b = n_blocks; b <= D3P_VAE_MAX_BLOCKS; ++b) f.w_off[b] = (uint32_t)N.P;
    return f;
}

// forward pass: activations, the reparametrised latent, da = sc (sigmoid(a) - x) and px_loss[i] = sc (log q - log p - log lik)
// eps != nullptr: given noise; otherwise drawn from jax_key inside k_vae_latent into ws.eps
// the nonce of the current exactness pass over the batch (per host thread: a forward pass and the weight-gradient products that
// follow it are enqueued by one thread, back to back)
static uint32_t vae_exact_nonce(bool advance)
{
    static thread_local uint32_t nonce = 0x5eed0000u;
    if (advance) ++nonce;
    return nonce;
}

// may the batch take the one-plane path at all (k_exact16_flag reads whole 16-byte words)?
static bool vae_exact_eligible(const float* X, uint32_t B, int D)
{
    static const bool no_exact = getenv("D3P_VAE_NO_EXACT16") != nullptr;   // developer switch (A/B), read once
    return !no_exact && ((size_t)B * D) % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15u) == 0;
}

static int vae_enqueue_forward(hipStream_t s, const d3p_vae_model* m, const float* params, const float* X, const uint8_t* mask,
                               uint32_t B, const float* eps, float sc, const VaeWorkspace& ws, const uint32_t* jax_key = nullptr,
                               uint32_t B_total = 0, uint32_t pos0 = 0, VaeStepPrep prep = VaeStepPrep(), const SiteNoiseArgs* noise = nullptr,
                               bool* out_fused = nullptr)
{
    // noise != nullptr: the Gaussian-mechanism noise of the update is drawn beside the latent kernel
    // out_fused != nullptr: the caller's norm kernel finishes a fused output layer (*out_fused says whether there is one: ws.ep_ll /
    // ws.ep_xx then hold per-group partial sums, px_loss / x2 do not exist yet); nullptr: px_loss and x2 are complete on return
    int rc;
    const VaeNet N = vae_net(m);
    const int D = N.D, Z = N.Z, HE = N.HE, nh = N.nh, Bi = (int)B;
    const dim3 rows(cdiv((uint64_t)B * 64, 256));
    // Is the batch exactly bf16 (binarised images, examples/vae.py:157-168)?  One pass over X (13 MB) decides for the two products
    // that take X as their A operand -- the first encoder layer and its weight gradient: they then stage one plane of A instead
    // of splitting it into three and issue three of the six products (GemmArgs::a_exact16).  Any other batch takes the general path.
    const uint32_t* xflag = nullptr;
    if (vae_exact_eligible(X, B, D)) {
        if (!prep.x_checked) {
            const size_t n4 = (size_t)B * D / 4;
            const uint32_t nonce = vae_exact_nonce(true);   // a new nonce per pass: the flag word is never reset
            exact16_flag_launch(s, X, n4, ws.x_exact16, nonce);
        }
        xflag = ws.x_exact16;
    }
    // ---- encoder (guide)
    {
        const float* in = X;
        for (int l = 0; l < nh; ++l) {
            const VaeDense& e = N.enc[l];
            GemmOpts o;   // softplus epilogue (sigmoid = its derivative to sge), split-K where the grid is short, one-plane A for the batch
            o.part = ws.part; o.part_floats = ws.part_floats; o.epi = 1; o.C2 = ws.sge[l];
            o.a_exact16 = l == 0 ? xflag : nullptr; o.a_exact_nonce = vae_exact_nonce(false);
            if ((rc = gemm(s, in, e.in, 1, params + e.W, e.out, 1, ws.he[l], e.out, Bi, e.out, e.in, params + e.b, 1.f, 0, o))) return rc;
            in = ws.he[l];
        }
    }
    // [z_loc | log z_std] = h [Wl | Ws] + [bl | bs] in ONE product of N = 2 Z: Ws lies HE Z behind where Wl's columns Z .. 2 Z - 1
    // would be, and bs likewise behind bl (flat layout: Wl, bl, Ws, bs)
    const int ldz = 2 * Z;
    // (packed heads: B = ws.wcat, a plain HE x 2 Z matrix -- only the bias keeps its displaced second half)
    const GemmJumps enc = {Z, 0x7fffffff, prep.heads_packed ? 0ll : (long long)HE * Z, 0, (long long)HE * Z, 0};
    // (a split-K product leaves its partial tiles for k_vae_latent to sum: no reduction launch)
    int zl_splits = 0;
    {
        GemmOpts o;
        o.part = ws.part; o.part_floats = ws.part_floats; o.splits_left = &zl_splits; o.jumps = &enc;
        if ((rc = gemm(s, ws.he[nh - 1], HE, 1, prep.heads_packed ? ws.wcat : params + N.Wl, prep.heads_packed ? 2 * Z : Z, 1, ws.zl, ldz, Bi, 2 * Z, HE,
                       params + N.bl, 1.f, 0, o)))
            return rc;
    }
    {
        LatentArgs la;
        memset(&la, 0, sizeof(la));
        la.zl = ws.zl; la.u = ws.u;   // zl := z, u := sd
        la.eps_in = eps; la.jax_key = eps ? (const uint32_t*)nullptr : jax_key;
        la.B_total = B_total ? B_total : B; la.pos0 = pos0;
        la.eps_out = ws.eps; la.B = B; la.Z = Z; la.ld = ldz; la.lat = ws.lat;
        la.part = ws.part; la.splits = zl_splits;
        la.bias_l = params + N.bl; la.bias_s = params + N.bs;
        if (noise) {
            la.noise = *noise;
            la.noise_blocks = cdiv(noise->blk_off[D3P_VAE_MAX_LEAVES], 256);
        }
        hipLaunchKernelGGL(k_vae_latent, dim3(rows.x + la.noise_blocks), dim3(256), 0, s, la);
    }
    // ---- decoder (model)
    {
        const float* in = ws.zl;
        int ld_in = ldz;
        for (int l = 0; l < nh; ++l) {
            const VaeDense& d = N.dec[l];
            // (the first product has K = Z: no split)
            GemmOpts o;
            o.part = l ? ws.part : nullptr; o.part_floats = l ? ws.part_floats : 0; o.epi = 1; o.C2 = ws.sgd[l];
            if ((rc = gemm(s, in, ld_in, 1, params + d.W, d.out, 1, ws.hd[l], d.out, Bi, d.out, d.in, params + d.b, 1.f, 0, o))) return rc;
            in = ws.hd[l];
            ld_in = d.out;
        }
        const VaeDense& o = N.dec[nh];
        // the output layer: when the product takes the bf16 kernel its epilogue does k_vae_out's work (GemmArgs::epi 4) instead of a
        // launch behind it
        static const bool no_fuse = getenv("D3P_VAE_NO_OUT_FUSE") != nullptr;   // developer switch (A/B), read once
        const int groups = (int)cdiv(D, 32);
        const bool fuse = !no_fuse && groups <= 64 && gemm_route(in, ld_in, 1, params + o.W, D, 1, Bi, D, o.in, 0, nullptr) == GEMM_ROUTE_BF16X3;
        if (out_fused) *out_fused = fuse;
        if (fuse) {
            GemmOpts go;
            go.epi = 4; go.ex_sc = sc; go.ep_x = X; go.ep_ll = ws.ep_ll; go.ep_xx = ws.ep_xx;
            if ((rc = gemm(s, in, ld_in, 1, params + o.W, D, 1, ws.a, D, Bi, D, o.in, params + o.b, 1.f, 0, go))) return rc;   // a := da
            if (!out_fused)
                hipLaunchKernelGGL(k_vae_out_finish, rows, dim3(256), 0, s, (const float*)ws.ep_ll, (const float*)ws.ep_xx, groups, B, (const float*)ws.lat,
                                   sc, mask, ws.px_loss, ws.x2);
            return check_launch("d3p_vae forward");
        }
        if ((rc = gemm(s, in, ld_in, 1, params + o.W, D, 1, ws.a, D, Bi, D, o.in, params + o.b, 1.f, 0))) return rc;
    }
    hipLaunchKernelGGL(k_vae_out, rows, dim3(256), 0, s, ws.a, X, mask, B, D, sc, (const float*)ws.lat, ws.px_loss, ws.x2);  // a := da
    return check_launch("d3p_vae forward");
}

// forward + backward + norms + clipped sums into ws.sums[P + 2]; eps_dev given or drawn from jax_key
// Data-parallel step (d3p_dpvi_vae_run_dist): the clipped sums leave the rank in TWO buckets, so that the reduce of the first
// travels while the products of the second still run.  (Every clipped sum needs the clip factors, i.e. the whole backward pass:
// what can overlap a reduce is the tail of the step -- the weight-gradient products, 63 of its 240 us at 4096 examples per rank.)
// Bucket 0 = the decoder's leaves (columns 0 .. split - 1 of the flat layout), bucket 1 = the encoder's and the latent heads' +
// [loss sum, count]; the weight-gradient products go out as one grouped launch per bucket, each followed by the tile sums of its
// columns and `ready(bucket)` (the caller enqueues the reduce behind an event).
// developer switch (A/B), read once: the weight-gradient products launched one by one.  The two-bucket hand-over exists only in the
// grouped form, so every caller that decides "two buckets" asks this predicate too (else no reduce would be enqueued at all).
static bool vae_no_group()
{
    static const bool v = getenv("D3P_VAE_NO_GROUP") != nullptr;
    return v;
}
struct VaeBuckets {
    size_t split;
    int (*ready)(void* ctx, int bucket);
    void* ctx;
};

static int vae_enqueue_sums(hipStream_t s, const d3p_vae_model* m, const float* params, const float* X, const uint8_t* mask,
                            uint32_t B, const float* eps_ext, const uint32_t* jax_key, float clip, const VaeWorkspace& ws,
                            float* norms_out, uint32_t B_total = 0, uint32_t pos0 = 0, int* w_splits = nullptr, VaeStepPrep prep = VaeStepPrep(),
                            const SiteNoiseArgs* noise = nullptr, bool* loss_pending = nullptr, const VaeBuckets* bk = nullptr)
{
    // The split-K partial tiles of the weight-gradient products stay in ws.wpart.  w_splits != nullptr (single-device update):
    // w_splits[0 .. n_blocks - 1] says how many each, and k_vae_finalize sums them; otherwise ONE launch (k_vae_tile_sums) sums
    // them into ws.sums here.
    if (B_total == 0) B_total = B;
    int rc;
    const VaeNet N = vae_net(m);
    const int D = N.D, Z = N.Z, HE = N.HE, nh = N.nh, Bi = (int)B;
    const float sc = m->inv_obs * m->scale;
    const float* eps = eps_ext ? eps_ext : ws.eps;  // (drawn inside k_vae_latent when not given)
    const dim3 rows(cdiv((uint64_t)B * 64, 256));
    // loss_pending (with w_splits, the single-device update): *loss_pending = the output layer was fused and ws.sums[P] is NOT the loss
    // sum -- the caller's k_vae_finalize takes it from ws.px_loss; without w_splits the tile-sum launch below does
    bool out_fused = false;
    if ((rc = vae_enqueue_forward(s, m, params, X, mask, B, eps_ext, sc, ws, jax_key, B_total, pos0, prep, noise, &out_fused))) return rc;
    // ---- backward (data): delta_in = (delta_out W^T) . softplus'(pre) down the decoder
    {
        const float* delta = ws.a;
        for (int l = nh - 1; l >= 0; --l) {
            const VaeDense& d = N.dec[l + 1];
            GemmOpts o;   // epilogue 2: times softplus'(pre)
            o.part = ws.part; o.part_floats = ws.part_floats; o.epi = 2; o.C2 = ws.sgd[l];
            if ((rc = gemm(s, delta, d.out, 1, params + d.W, 1, d.out, ws.dd[l], d.in, Bi, d.in, d.out, nullptr, 1.f, 0, o))) return rc;
            delta = ws.dd[l];
        }
    }
    const int ldz = 2 * Z;
    // dz = dpre V1^T + sc z and du = dz sd eps - sc in the product's epilogue (epi 3; was the k_vae_dlatent launch)
    {
        GemmOpts o;
        o.part = ws.part; o.part_floats = ws.part_floats; o.epi = 3; o.ex_zu = ws.zl; o.ex_eps = eps; o.ex_Z = Z; o.ex_sc = sc;
        if ((rc = gemm(s, ws.dd[0], N.dec[0].out, 1, params + N.dec[0].W, 1, N.dec[0].out, ws.dz, ldz, Bi, Z, N.dec[0].out, nullptr, 1.f, 0, o))) return rc;
    }
    // dpre = ([dz | du] [Wl^T ; Ws^T]) . softplus'(pre): ONE product of K = 2 Z (rows Z .. 2 Z - 1 of the stacked B are Ws^T,
    // HE Z behind where Wl^T's would be)
    // (packed heads: B = ws.wcatT, a plain 2 Z x HE matrix with 16-byte rows -- the product takes the bf16 kernel)
    const GemmJumps dec = {0x7fffffff, Z, 0, (long long)HE * Z, 0, 0};
    {
        GemmOpts o;
        o.epi = 2; o.C2 = ws.sge[nh - 1];
        if (prep.heads_packed) {
            rc = gemm(s, ws.dz, ldz, 1, ws.wcatT, HE, 1, ws.de[nh - 1], HE, Bi, HE, 2 * Z, nullptr, 1.f, 0, o);
        } else {
            o.jumps = &dec;
            rc = gemm(s, ws.dz, ldz, 1, params + N.Wl, 1, Z, ws.de[nh - 1], HE, Bi, HE, 2 * Z, nullptr, 1.f, 0, o);
        }
        if (rc) return rc;
    }
    for (int l = nh - 2; l >= 0; --l) {
        const VaeDense& e = N.enc[l + 1];
        GemmOpts o;
        o.part = ws.part; o.part_floats = ws.part_floats; o.epi = 2; o.C2 = ws.sge[l];
        if ((rc = gemm(s, ws.de[l + 1], e.out, 1, params + e.W, 1, e.out, ws.de[l], e.in, Bi, e.in, e.out, nullptr, 1.f, 0, o))) return rc;
    }
    // ---- clipped sums: weights  A^T (diag(c) Delta)  (GEMMs over the batch), biases = column sums
    // [W | b] of every layer is contiguous in the flat layout, so the bias gradient is row `in` of a GEMM whose A carries a
    // virtual row of ones
    float* S = ws.sums;
    // one product per dense layer (decoder, then encoder), then ONE for [Wl | Ws] (B operand [dz | du], N = 2 Z; the Ws block of
    // the sums lies HE Z behind where columns Z .. 2 Z - 1 of a Z-wide C would be)
    struct WG { const float* A; long long a_sk; int in; const float* Bm; int ldb; int out; int ldc; size_t off; const GemmJumps* j; int blk; };
    const GemmJumps wls = {Z, 0x7fffffff, 0, 0, 0, (long long)HE * Z};
    WG wg[6];
    int n_wg = 0;
    for (int l = 0; l <= nh; ++l) {
        const VaeDense& d = N.dec[l];
        wg[n_wg++] = {l == 0 ? ws.zl : ws.hd[l - 1], l == 0 ? ldz : d.in, d.in, l == nh ? ws.a : ws.dd[l], d.out, d.out, d.out, d.W, nullptr, l};
    }
    for (int l = 0; l < nh; ++l) {
        const VaeDense& e = N.enc[l];
        wg[n_wg++] = {l == 0 ? X : ws.he[l - 1], e.in, e.in, ws.de[l], e.out, e.out, e.out, e.W, nullptr, nh + 1 + l};
    }
    wg[n_wg++] = {ws.he[nh - 1], HE, HE, ws.dz, ldz, 2 * Z, Z, N.Wl, &wls, 2 * nh + 1};
    // Where do the clip factors meet the deltas?  When every product takes the bf16 kernel it multiplies the rows of its B operand by
    // c_i while staging them (GemmArgs::b_row_scale) and the norm kernel only reads; otherwise the norm kernel writes the rows back scaled.
    static const bool scale_back_env = getenv("D3P_VAE_SCALE_BACK") != nullptr;   // developer switch (A/B), read once
    bool scale_in_gemm = !scale_back_env;
    for (int b = 0; b < n_wg; ++b)
        scale_in_gemm = scale_in_gemm && gemm_route(wg[b].A, 1, wg[b].a_sk, wg[b].Bm, wg[b].ldb, 1, wg[b].in + 1, wg[b].out, Bi, 1, wg[b].j) == GEMM_ROUTE_BF16X3;
    // ---- per-example norms and clip factors (and, unless scale_in_gemm, the rows of every delta come back scaled by c_i)
    NormArgs na;
    memset(&na, 0, sizeof(na));
    na.scale_back = scale_in_gemm ? 0 : 1;
    {
        int t = 0;
        auto term = [&](const float* in, int in_ld, int in_n, float* d0, float* d1, int d_ld, int d_n) {
            NormTerm& q = na.t[t++];
            q.in = in; q.in_ld = in_ld; q.in_n = in_n; q.d0 = d0; q.d1 = d1; q.d_ld = d_ld; q.d_n = d_n;
            na.stage += ((d_n + 3) & ~3) * (d1 ? 2 : 1);   // (every row of the stage starts on a 16-byte boundary)
        };
        term(ws.hd[nh - 1], N.dec[nh].in, N.dec[nh].in, ws.a, nullptr, D, D);
        for (int l = nh - 1; l >= 1; --l) term(ws.hd[l - 1], N.dec[l].in, N.dec[l].in, ws.dd[l], nullptr, N.dec[l].out, N.dec[l].out);
        term(ws.zl, ldz, Z, ws.dd[0], nullptr, N.dec[0].out, N.dec[0].out);
        term(ws.he[nh - 1], HE, HE, ws.dz, ws.du, ldz, Z);
        for (int l = nh - 1; l >= 1; --l) term(ws.he[l - 1], N.enc[l].in, N.enc[l].in, ws.de[l], nullptr, N.enc[l].out, N.enc[l].out);
        term(nullptr, 0, 0, ws.de[0], nullptr, N.enc[0].out, N.enc[0].out);
        na.n_terms = t;
    }
    na.x2 = ws.x2;
    na.mask = mask; na.B = B; na.clip = clip; na.cf = ws.cf; na.norms = norms_out;
    na.px_loss = ws.px_loss; na.loss_n = ws.sums + N.P;
    if (out_fused) { na.ep_ll = ws.ep_ll; na.ep_xx = ws.ep_xx; na.lat = ws.lat; na.ep_groups = (int)cdiv(D, 32); na.ep_sc = sc; }
    {
        size_t stage_floats = na.scale_back ? 4 * (size_t)na.stage : 0;
        if (stage_floats < 512) stage_floats = 512;  // the last workgroup's loss / count reduction uses 2 x 256 floats
        hipLaunchKernelGGL(k_vae_norms, dim3(rows.x + 1), dim3(256), stage_floats * sizeof(float), s, na);
    }
    // single-device update: the products go out as ONE grouped launch with a common K range per workgroup
    // (bk: one grouped launch per bucket)
    const bool no_group = vae_no_group();
    int splits_here[D3P_VAE_MAX_BLOCKS] = {0};
    int* const tile_splits = w_splits ? w_splits : splits_here;
    bool loss_summed = false;   // (fused output layer: a group launch sums px_loss into S[P] beside its products)
    const int n_buckets = (bk && !no_group) ? 2 : 1;
    for (int bucket = 0; bucket < n_buckets; ++bucket) {
        auto in_bucket = [&](int b) { return n_buckets == 1 || (bucket == 0) == (wg[b].off < bk->split); };
        GemmGroupPlan plan;
        GemmGroupPlan* group = !no_group ? &plan : nullptr;
        int group_splits = 0;
        if (group) {
            unsigned tiles = 0;
            for (int b = 0; b < n_wg; ++b)
                if (in_bucket(b)) tiles += cdiv(wg[b].out, D3P_GT) * cdiv(wg[b].in + 1, D3P_GTM);
            group_splits = gemm_group_splits(tiles, Bi);
        }
        for (int b = 0; b < n_wg; ++b) {
            if (!in_bucket(b)) continue;
            float* part = ws.wpart + (size_t)D3P_WPART_SPLITS * wg[b].off;
            const size_t part_floats = (size_t)D3P_WPART_SPLITS * (wg[b].in + 1) * wg[b].out;
            int left = 0;
            // (A = X^T: the flag of the forward pass holds -- same batch; the virtual row of ones is exact too)
            const uint32_t* xflag = (wg[b].A == X && vae_exact_eligible(X, B, D)) ? ws.x_exact16 : nullptr;
            GemmOpts o;   // A carries the virtual row of ones (bias gradient); tiles left unreduced; grouped; clip factors on B's rows
            o.a_last_one = 1; o.part = part; o.part_floats = part_floats; o.splits_left = &left; o.jumps = wg[b].j;
            o.a_exact16 = xflag; o.a_exact_nonce = vae_exact_nonce(false);
            o.group = group; o.force_splits = group_splits; o.b_row_scale = scale_in_gemm ? ws.cf : nullptr;
            if ((rc = gemm(s, wg[b].A, 1, wg[b].a_sk, wg[b].Bm, wg[b].ldb, 1, S + wg[b].off, wg[b].ldc, wg[b].in + 1, wg[b].out, Bi, nullptr, 1.f, 0, o)))
                return rc;
            tile_splits[wg[b].blk] = left;
            if (b == n_wg - 1) tile_splits[wg[b].blk + 1] = left;
        }
        const bool last = bucket == n_buckets - 1;
        if (group && out_fused && plan.n > 0 && last) {
            plan.sum_in = ws.px_loss; plan.sum_out = S + N.P; plan.sum_n = B;
            loss_summed = true;
        }
        if (group && (rc = gemm_group_launch(s, plan))) return rc;
        if (!w_splits) {
            const size_t c0 = (n_buckets == 2 && bucket == 1) ? bk->split : 0, c1 = (n_buckets == 2 && bucket == 0) ? bk->split : (size_t)N.P;
            hipLaunchKernelGGL(k_vae_tile_sums, dim3(cdiv(c1 - c0, 256)), dim3(256), 0, s, vae_tiles(N, ws, tile_splits), S, N.P,
                               (last && out_fused && !loss_summed) ? (const float*)ws.px_loss : (const float*)nullptr, B, c0, c1);
            if (n_buckets == 2 && (rc = bk->ready(bk->ctx, bucket))) return rc;
        }
    }
    if (loss_pending) *loss_pending = out_fused && !loss_summed;
    return check_launch("d3p_vae sums");
}

// ---- predictive sampling (d3p_predict.hip): the guide's encoder and the model's decoder as plain forward passes through the
// product kernels above (softplus layers: epilogue 1, its sigmoid output to `sg`, unused); no split-K.
// encoder: zl = h Wl + bl, zs = h Ws + bs (the log of the guide's z_std, examples/vae.py:86) over the B rows of X
int vae_predict_encode(hipStream_t s, const d3p_vae_model* m, const float* params, const float* X, uint32_t B, float* zl, float* zs, float* h0, float* h1,
                       float* sg)
{
    const VaeNet N = vae_net(m);
    const int Bi = (int)B, Z = N.Z, HE = N.HE;
    const float* in = X;
    float* bufs[2] = {h0, h1};
    for (int l = 0; l < N.nh; ++l) {
        const VaeDense& e = N.enc[l];
        GemmOpts o;
        o.epi = 1; o.C2 = sg;
        if (int rc = gemm(s, in, e.in, 1, params + e.W, e.out, 1, bufs[l], e.out, Bi, e.out, e.in, params + e.b, 1.f, 0, o)) return rc;
        in = bufs[l];
    }
    if (int rc = gemm(s, in, HE, 1, params + N.Wl, Z, 1, zl, Z, Bi, Z, HE, params + N.bl, 1.f, 0)) return rc;
    return gemm(s, in, HE, 1, params + N.Ws, Z, 1, zs, Z, Bi, Z, HE, params + N.bs, 1.f, 0);
}

// decoder: logits = the output layer's pre-activation (rows x D) for the rows of z (rows x Z); the model's sigmoid is applied by the
// Bernoulli draw that reads them
int vae_predict_decode(hipStream_t s, const d3p_vae_model* m, const float* params, const float* z, uint32_t rows, float* logits, float* h0, float* h1,
                       float* sg)
{
    const VaeNet N = vae_net(m);
    const int R = (int)rows;
    const float* in = z;
    int ld_in = N.Z;
    float* bufs[2] = {h0, h1};
    for (int l = 0; l < N.nh; ++l) {
        const VaeDense& d = N.dec[l];
        GemmOpts o;
        o.epi = 1; o.C2 = sg;
        if (int rc = gemm(s, in, ld_in, 1, params + d.W, d.out, 1, bufs[l], d.out, R, d.out, d.in, params + d.b, 1.f, 0, o)) return rc;
        in = bufs[l];
        ld_in = d.out;
    }
    const VaeDense& o = N.dec[N.nh];
    return gemm(s, in, ld_in, 1, params + o.W, o.out, 1, logits, o.out, R, o.out, o.in, params + o.b, 1.f, 0);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

int64_t d3p_vae_num_params(const d3p_vae_model* model)
{
    if (!model || model->D < 1 || model->H < 1 || model->Z < 1 || model->H2 < 0) return 0;
    return (int64_t)vae_net(model).P;
}

size_t d3p_dpvi_vae_workspace(const d3p_vae_model* model, uint32_t B)
{
    if (!model || model->D < 1 || model->H < 1 || model->Z < 1 || model->H2 < 0) return 0;
    return vae_carve(model, B, nullptr, nullptr);
}

int d3p_vae_step_sums(void* stream, const d3p_vae_model* model, const float* params_dev, const float* X_dev, const uint8_t* mask_dev,
                      uint32_t B, const float* eps_dev, const uint32_t* jax_key_dev, float clip, float* sums_dev, float* norms_dev,
                      float* px_loss_dev, void* workspace_dev, size_t workspace_bytes)
{
    if (int rc = vae_validate(model, "d3p_vae_step_sums")) return rc;
    D3P_REQUIRE(params_dev && X_dev && sums_dev && workspace_dev && (eps_dev || jax_key_dev), "d3p_vae_step_sums: null pointer");
    D3P_REQUIRE(B >= 1 && clip > 0.f, "d3p_vae_step_sums: B >= 1 and clip > 0 required");
    if (workspace_bytes < d3p_dpvi_vae_workspace(model, B)) return fail(D3P_E_WORKSPACE, "d3p_vae_step_sums: workspace too small");
    VaeWorkspace ws;
    vae_carve(model, B, (char*)workspace_dev, &ws);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = vae_enqueue_sums(s, model, params_dev, X_dev, mask_dev, B, eps_dev, jax_key_dev, clip, ws, norms_dev)) return rc;
    const size_t P = vae_net(model).P;
    D3P_HIP_TRY(hipMemcpyAsync(sums_dev, ws.sums, (P + 2) * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (px_loss_dev) D3P_HIP_TRY(hipMemcpyAsync(px_loss_dev, ws.px_loss, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, s));
    return D3P_OK;
}

int d3p_vae_evaluate(void* stream, const d3p_vae_model* model, const float* params_dev, const float* X_dev, uint32_t B,
                     const uint32_t* jax_key_dev, const float* eps_dev, float* loss_dev, void* workspace_dev, size_t workspace_bytes)
{
    if (int rc = vae_validate(model, "d3p_vae_evaluate")) return rc;
    D3P_REQUIRE(params_dev && X_dev && loss_dev && workspace_dev && (jax_key_dev || eps_dev), "d3p_vae_evaluate: null pointer");
    D3P_REQUIRE(B >= 1, "d3p_vae_evaluate: B must be >= 1");
    if (workspace_bytes < d3p_dpvi_vae_workspace(model, B)) return fail(D3P_E_WORKSPACE, "d3p_vae_evaluate: workspace too small");
    VaeWorkspace ws;
    vae_carve(model, B, (char*)workspace_dev, &ws);
    hipStream_t s = (hipStream_t)stream;
    const float* eps = eps_dev;
    if (!eps) {
        hipLaunchKernelGGL(k_vae_eval_eps, dim3(cdiv((uint64_t)B * model->Z, 256)), dim3(256), 0, s, jax_key_dev, B, model->Z, ws.eps);
        eps = ws.eps;
    }
    if (int rc = vae_enqueue_forward(s, model, params_dev, X_dev, nullptr, B, eps, model->inv_obs * model->scale, ws)) return rc;
    const size_t P = vae_net(model).P;
    hipLaunchKernelGGL(k_vae_loss_n, dim3(1), dim3(256), 0, s, (const float*)ws.px_loss, (const uint8_t*)nullptr, B, ws.sums + P);
    D3P_HIP_TRY(hipMemcpyAsync(loss_dev, ws.sums + P, sizeof(float), hipMemcpyDeviceToDevice, s));
    return check_launch("d3p_vae_evaluate");
}

static int vae_update_checks(const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                             const void* workspace_dev, const char* what)
{
    if (int rc = vae_validate(model, what)) return rc;
    if (!(hyper && state && state->rng_key && state->params && state->adam_m && state->adam_v && state->step && workspace_dev))
        return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if (!(hyper->clip > 0.f) || !std::isfinite(hyper->clip))
        return fail(D3P_E_INVALID_ARG, "%s: the clipping threshold must be finite and greater than 0", what);
    return D3P_OK;
}

// keys of one update, all functions of the state key: [next | gradient | perturbation] = split(key, 3) (svi.py:208-211),
// split(perturbation_key, 10) (svi.py:491), convert_to_jax_rng_key(gradient_key)
// from != nullptr: the update reads the key and the step counter of `from` and writes the next key / counter into `state`
// (slot 1 of its key buffer; state->key_slot is taken as 0)
// X != nullptr (with prep): the exactness pass over the batch the forward pass is about to take, and the packing of the latent
// heads of `params` (the parameters that pass runs on), ride in this launch; *prep says which of them did
static int vae_step_keys(hipStream_t s, const d3p_vae_model* model, const d3p_dpsvi_state* state, const VaeWorkspace& ws, bool advance,
                         const d3p_dpsvi_state* from = nullptr, const float* X = nullptr, uint32_t B = 0, const float* params = nullptr,
                         VaeStepPrep* prep = nullptr, const VaeRunStep* rs = nullptr)
{
    // rs != nullptr (the run loop): X is the batch buffer the step's rows are ABOUT to be gathered into -- this launch makes the
    // indices, the caller gathers (and checks exactness) behind it
    const VaeNet N = vae_net(model);
    const int slot = state->key_slot & 1, n_sites = N.n_leaves();
    KeysExtra ex;
    memset(&ex, 0, sizeof(ex));
    unsigned pack_blocks = 0, feistel_blocks = 0;
    if (rs) {
        int bits = 0;   // bit_length(n_rows - 1), util.py:230
        for (uint32_t v = rs->n_rows - 1; v; v >>= 1) ++bits;
        ex.batch_key = rs->batch_key; ex.batch_i = rs->batch_i; ex.capacity = rs->n_rows; ex.n_idx = B;
        ex.bits_lower = bits >> 1; ex.bits_upper = bits - (bits >> 1);
        ex.idx = rs->idx;
        feistel_blocks = cdiv(B, 256);
    } else if (X && prep && vae_exact_eligible(X, B, model->D)) {
        ex.x = X;
        ex.x_n4 = (size_t)B * model->D / 4;
        ex.x_flag = ws.x_exact16;
        ex.x_nonce = vae_exact_nonce(true);
        ex.x_blocks = exact16_blocks(ex.x_n4);
        prep->x_checked = true;
    }
    static const bool no_pack = getenv("D3P_VAE_NO_HEAD_PACK") != nullptr;   // developer switch (A/B), read once
    if (params && prep && !no_pack && (2 * N.Z) % 4 == 0 && N.HE % 4 == 0) {
        ex.wl = params + N.Wl; ex.wsd = params + N.Ws;
        ex.wcat = ws.wcat; ex.wcatT = ws.wcatT;
        ex.HE = N.HE; ex.Z = N.Z;
        pack_blocks = cdiv((uint64_t)N.HE * 2 * N.Z, 256);
        prep->heads_packed = true;
    }
    ex.pack_blocks = pack_blocks;
    const dim3 grid(1 + ex.x_blocks + pack_blocks + feistel_blocks);
    if (from)
        hipLaunchKernelGGL(k_vae_keys, grid, dim3(256), 0, s, (const uint32_t*)(from->rng_key + 16 * (from->key_slot & 1)), ws.keys,
                           state->rng_key + 16, (const int32_t*)from->step, state->step, advance ? 1 : 0, n_sites, ex);
    else
        hipLaunchKernelGGL(k_vae_keys, grid, dim3(256), 0, s, (const uint32_t*)(state->rng_key + 16 * slot), ws.keys,
                           state->rng_key + 16 * (slot ^ 1), (const int32_t*)state->step, state->step, advance ? 1 : 0, n_sites, ex);
    return check_launch("k_vae_keys");
}

// the Gaussian-mechanism noise of an update: one key per leaf, normal(site_key, leaf shape) (svi.py:487)
static SiteNoiseArgs vae_site_noise_args(const VaeNet& N, const VaeWorkspace& ws)
{
    size_t leaf_off[D3P_VAE_MAX_LEAVES + 1];
    int k = 0;
    for (int l = 0; l <= N.nh; ++l) { leaf_off[k++] = N.dec[l].W; leaf_off[k++] = N.dec[l].b; }
    for (int l = 0; l < N.nh; ++l) { leaf_off[k++] = N.enc[l].W; leaf_off[k++] = N.enc[l].b; }
    leaf_off[k++] = N.Wl; leaf_off[k++] = N.bl; leaf_off[k++] = N.Ws; leaf_off[k++] = N.bs;
    for (; k <= D3P_VAE_MAX_LEAVES; ++k) leaf_off[k] = N.P;
    SiteNoiseArgs na;
    na.site_keys = ws.keys + 48;
    na.noise = ws.noise;
    na.blk_off[0] = 0;
    for (k = 0; k < D3P_VAE_MAX_LEAVES; ++k) {
        na.elem_off[k] = (uint32_t)leaf_off[k];
        na.blk_off[k + 1] = na.blk_off[k] + (uint32_t)((leaf_off[k + 1] - leaf_off[k] + 15) / 16);
    }
    na.elem_off[D3P_VAE_MAX_LEAVES] = (uint32_t)leaf_off[D3P_VAE_MAX_LEAVES];
    return na;
}

static int vae_apply_impl(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                          const float* sums_dev, uint32_t B_total, uint32_t B_local, float* loss_dev, float* grad_out_dev,
                          void* workspace_dev, size_t workspace_bytes, bool derive_keys, const int* w_splits = nullptr,
                          const d3p_dpsvi_state* from = nullptr, bool loss_pending = false, bool noise_drawn = false);

// advance = true (single-device update): the key kernel also writes the next state key and advances the step counter, so that
// vae_apply_impl(derive_keys = false) has nothing left to launch for them
static int vae_local_sums_impl(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                               const float* X_dev, const uint8_t* mask_dev, uint32_t B_local, uint32_t B_total, uint32_t pos0,
                               const float* eps_dev, float* sums_dev, void* workspace_dev, size_t workspace_bytes, bool advance,
                               int* w_splits = nullptr, const d3p_dpsvi_state* from = nullptr, const VaeRunStep* rs = nullptr,
                               bool* loss_pending = nullptr, bool draw_noise = false, const VaeBuckets* bk = nullptr)
{
    // draw_noise (with advance; the native data-parallel loop): the Gaussian-mechanism noise of the update is drawn beside the latent
    // kernel although the sums leave the device function for a reduce -- it depends on the step's keys only
    // rs != nullptr: X_dev is the batch BUFFER; the step's rows are gathered into it here (indices from the key launch)
    // loss_pending (with w_splits): vae_enqueue_sums' -- the caller hands it on to vae_apply_impl
    if (int rc = vae_update_checks(model, hyper, state, workspace_dev, "d3p_dpvi_vae_local_sums")) return rc;
    D3P_REQUIRE(X_dev && sums_dev, "d3p_dpvi_vae_local_sums: null pointer");
    D3P_REQUIRE(B_local >= 1 && (uint64_t)pos0 + B_local <= B_total, "d3p_dpvi_vae_local_sums: need 1 <= B_local and pos0 + B_local <= B_total");
    if (workspace_bytes < d3p_dpvi_vae_workspace(model, B_local)) return fail(D3P_E_WORKSPACE, "d3p_dpvi_vae_local_sums: workspace too small");
    VaeWorkspace ws;
    vae_carve(model, B_local, (char*)workspace_dev, &ws);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    VaeStepPrep prep;
    if ((rc = vae_step_keys(s, model, state, ws, advance, from, X_dev, B_local, from ? from->params : state->params, &prep, rs))) return rc;
    if (rs) {   // gather + exactness pass in one sweep (d3p_take_rows and k_exact16_flag's work)
        const bool chk = vae_exact_eligible(X_dev, B_local, model->D);
        const uint32_t d4 = (uint32_t)model->D / 4;
        const size_t n = (size_t)B_local * d4;
        hipLaunchKernelGGL(k_vae_gather_check, dim3((unsigned)(n / 512 < 1 ? 1 : (n / 512 > 2048 ? 2048 : n / 512))), dim3(256), 0, s, rs->table,
                           (const uint32_t*)rs->idx, B_local, d4, const_cast<float*>(X_dev), chk ? ws.x_exact16 : (uint32_t*)nullptr,
                           chk ? vae_exact_nonce(true) : 0u);
        prep.x_checked = chk;
    }
    // w_splits != nullptr = the single-device update: vae_apply_impl follows on the same workspace with these keys, so its noise is
    // drawn here, beside the latent kernel
    const SiteNoiseArgs noise = vae_site_noise_args(vae_net(model), ws);
    if ((rc = vae_enqueue_sums(s, model, from ? from->params : state->params, X_dev, mask_dev, B_local, eps_dev, ws.keys + D3P_VAE_KEY_JAX, hyper->clip, ws, nullptr,
                               B_total, pos0, w_splits, prep, (w_splits || draw_noise) ? &noise : nullptr, w_splits ? loss_pending : nullptr, bk)))
        return rc;
    if (sums_dev != ws.sums)
        D3P_HIP_TRY(hipMemcpyAsync(sums_dev, ws.sums, (vae_net(model).P + 2) * sizeof(float), hipMemcpyDeviceToDevice, s));
    return check_launch("d3p_dpvi_vae_local_sums");
}

int d3p_dpvi_vae_local_sums(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                            const float* X_dev, const uint8_t* mask_dev, uint32_t B_local, uint32_t B_total, uint32_t pos0,
                            const float* eps_dev, float* sums_dev, void* workspace_dev, size_t workspace_bytes)
{
    return vae_local_sums_impl(stream, model, hyper, state, X_dev, mask_dev, B_local, B_total, pos0, eps_dev, sums_dev, workspace_dev,
                               workspace_bytes, false);
}

int d3p_dpvi_vae_apply(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                       const float* sums_dev, uint32_t B_total, uint32_t B_local, float* loss_dev, float* grad_out_dev,
                       void* workspace_dev, size_t workspace_bytes)
{
    return vae_apply_impl(stream, model, hyper, state, sums_dev, B_total, B_local, loss_dev, grad_out_dev, workspace_dev,
                          workspace_bytes, true);
}

// the arguments of the update of one step (k_vae_finalize, k_vae_fmesh_step)
static VaeFinalArgs vae_final_args(const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state, const VaeWorkspace& ws,
                                   const float* sums_dev, uint32_t B_total, uint32_t B_local, float* loss_dev, float* grad_out_dev, const int* w_splits,
                                   const d3p_dpsvi_state* from, bool loss_pending)
{
    const VaeNet N = vae_net(model);
    VaeFinalArgs f;
    memset(&f, 0, sizeof(f));
    f.sums = sums_dev;
    f.tiles = vae_tiles(N, ws, w_splits);
    f.noise = ws.noise;
    f.in_params = from ? from->params : state->params;
    f.in_m = from ? from->adam_m : state->adam_m;
    f.in_v = from ? from->adam_v : state->adam_v;
    f.params = state->params;
    f.adam_m = state->adam_m;
    f.adam_v = state->adam_v;
    f.step = reinterpret_cast<const int32_t*>(ws.keys + D3P_VAE_KEY_STEP);  // the step index k_vae_keys saved before advancing it
    f.loss_out = loss_dev;
    f.grad_out = grad_out_dev;
    f.P = N.P;
    f.B = B_total;
    f.h = *hyper;
    f.obs_scale = 1.0f / model->inv_obs;
    f.px_loss = loss_pending ? ws.px_loss : nullptr;
    f.B_local = B_local;
    return f;
}

// derive_keys = false: the keys of this update are already in the workspace (left there by d3p_dpvi_vae_local_sums on the same
// workspace and state, as in the single-device update)
static int vae_apply_impl(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                          const float* sums_dev, uint32_t B_total, uint32_t B_local, float* loss_dev, float* grad_out_dev,
                          void* workspace_dev, size_t workspace_bytes, bool derive_keys, const int* w_splits, const d3p_dpsvi_state* from,
                          bool loss_pending, bool noise_drawn)
{
    // loss_pending (single-device update): sums_dev[P] does not hold the loss sum -- k_vae_finalize takes it from ws.px_loss
    if (int rc = vae_update_checks(model, hyper, state, workspace_dev, "d3p_dpvi_vae_apply")) return rc;
    D3P_REQUIRE(sums_dev && B_total >= 1 && B_local >= 1, "d3p_dpvi_vae_apply: null pointer or empty batch");
    if (workspace_bytes < d3p_dpvi_vae_workspace(model, B_local)) return fail(D3P_E_WORKSPACE, "d3p_dpvi_vae_apply: workspace too small");
    VaeWorkspace ws;
    vae_carve(model, B_local, (char*)workspace_dev, &ws);
    hipStream_t s = (hipStream_t)stream;
    const VaeNet N = vae_net(model);
    int rc;
    if (derive_keys && (rc = vae_step_keys(s, model, state, ws, true))) return rc;
    if (derive_keys || (!w_splits && !noise_drawn)) {  // (the single-device update and the native data-parallel loop drew the noise beside their latent kernel: vae_local_sums_impl)
        const SiteNoiseArgs na = vae_site_noise_args(N, ws);
        hipLaunchKernelGGL(k_vae_site_noise, dim3(cdiv(na.blk_off[D3P_VAE_MAX_LEAVES], 256)), dim3(256), 0, s, na);
    }
    const VaeFinalArgs f = vae_final_args(model, hyper, state, ws, sums_dev, B_total, B_local, loss_dev, grad_out_dev, w_splits, from, loss_pending);
    hipLaunchKernelGGL(k_vae_finalize, dim3(cdiv(N.P, 256)), dim3(256), 0, s, f);
    return check_launch("d3p_dpvi_vae_apply");
}

// d3p_dpvi_vae_update as a function of an immutable state: reads `from` (key slot from->key_slot, parameters, Adam moments, step
// counter), writes the new state into `state` (its arrays may be uninitialised; the next key goes to slot 1 of state->rng_key)
// -- no copy of the 3 x 689 k floats of state per update.
int d3p_dpvi_vae_update_from(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                             const d3p_dpsvi_state* from, const float* X_dev, const uint8_t* mask_dev, uint32_t B, const float* eps_dev,
                             float* loss_dev, float* grad_out_dev, void* workspace_dev, size_t workspace_bytes)
{
    if (int rc = vae_update_checks(model, hyper, state, workspace_dev, "d3p_dpvi_vae_update_from")) return rc;
    D3P_REQUIRE(from && from->rng_key && from->params && from->adam_m && from->adam_v && from->step, "d3p_dpvi_vae_update_from: null source state");
    D3P_REQUIRE(X_dev, "d3p_dpvi_vae_update_from: null pointer");
    D3P_REQUIRE(B >= 1, "d3p_dpvi_vae_update_from: B must be >= 1");
    D3P_REQUIRE(state->key_slot == 0, "d3p_dpvi_vae_update_from: state->key_slot must be 0");
    if (workspace_bytes < d3p_dpvi_vae_workspace(model, B)) return fail(D3P_E_WORKSPACE, "d3p_dpvi_vae_update_from: workspace too small");
    VaeWorkspace ws;
    vae_carve(model, B, (char*)workspace_dev, &ws);
    int w_splits[D3P_VAE_MAX_BLOCKS];
    bool loss_pending = false;
    if (int rc = vae_local_sums_impl(stream, model, hyper, state, X_dev, mask_dev, B, B, 0, eps_dev, ws.sums, workspace_dev,
                                     workspace_bytes, true, w_splits, from, nullptr, &loss_pending))
        return rc;
    return vae_apply_impl(stream, model, hyper, state, ws.sums, B, B, loss_dev, grad_out_dev, workspace_dev, workspace_bytes, false,
                          w_splits, from, loss_pending);
}

static int vae_update_impl(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                           const float* X_dev, const uint8_t* mask_dev, uint32_t B, const float* eps_dev, float* loss_dev,
                           float* grad_out_dev, void* workspace_dev, size_t workspace_bytes, const VaeRunStep* rs)
{
    // the single-device update IS the data-parallel one with one rank: local sums, (no reduce), apply
    if (int rc = vae_update_checks(model, hyper, state, workspace_dev, "d3p_dpvi_vae_update")) return rc;
    D3P_REQUIRE(X_dev, "d3p_dpvi_vae_update: null pointer");
    D3P_REQUIRE(B >= 1, "d3p_dpvi_vae_update: B must be >= 1");
    if (workspace_bytes < d3p_dpvi_vae_workspace(model, B)) return fail(D3P_E_WORKSPACE, "d3p_dpvi_vae_update: workspace too small");
    VaeWorkspace ws;
    vae_carve(model, B, (char*)workspace_dev, &ws);
    int w_splits[D3P_VAE_MAX_BLOCKS];  // split-K partial tiles of the weight gradients are summed by k_vae_finalize, not by reduction launches
    bool loss_pending = false;
    if (int rc = vae_local_sums_impl(stream, model, hyper, state, X_dev, mask_dev, B, B, 0, eps_dev, ws.sums, workspace_dev,
                                     workspace_bytes, true, w_splits, nullptr, rs, &loss_pending))
        return rc;
    return vae_apply_impl(stream, model, hyper, state, ws.sums, B, B, loss_dev, grad_out_dev, workspace_dev, workspace_bytes, false,
                          w_splits, nullptr, loss_pending);
}

int d3p_dpvi_vae_update(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                        const float* X_dev, const uint8_t* mask_dev, uint32_t B, const float* eps_dev, float* loss_dev,
                        float* grad_out_dev, void* workspace_dev, size_t workspace_bytes)
{
    return vae_update_impl(stream, model, hyper, state, X_dev, mask_dev, B, eps_dev, loss_dev, grad_out_dev, workspace_dev, workspace_bytes,
                           nullptr);
}

// num_steps x (get_batch(first_batch + t, batch_key) of subsample_batchify_data -> update) on the resident data set X_dev
// (n_rows x D): the body of the example's jit(fori_loop(...)) epoch (examples/vae.py:227-246) -- per step fold_in, the Feistel
// indices, the row gather into xb_dev (B x D) and the update, all enqueued back to back: no host work depends on a result.
// `state` is advanced in place (its key_slot field says which slot of state->rng_key holds the key BEFORE the run; afterwards
// the key is in slot (key_slot + num_steps) & 1).  idx_dev: B uint32 + 16 (the step's batch key).
int d3p_dpvi_vae_run(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                     const uint32_t* batch_key_dev, uint32_t first_batch, const float* X_dev, uint32_t n_rows, uint32_t B,
                     uint32_t num_steps, float* losses_dev, float* xb_dev, uint32_t* idx_dev, void* workspace_dev, size_t workspace_bytes)
{
    if (int rc = vae_update_checks(model, hyper, state, workspace_dev, "d3p_dpvi_vae_run")) return rc;
    D3P_REQUIRE(batch_key_dev && X_dev && xb_dev && idx_dev, "d3p_dpvi_vae_run: null pointer");
    D3P_REQUIRE(B >= 1 && B <= n_rows, "d3p_dpvi_vae_run: need 1 <= B <= n_rows");
    if (workspace_bytes < d3p_dpvi_vae_workspace(model, B)) return fail(D3P_E_WORKSPACE, "d3p_dpvi_vae_run: workspace too small");
    d3p_dpsvi_state st = *state;
    uint32_t* step_key = idx_dev + B;
    // 16-byte rows: the step's indices come out of its key launch and ONE sweep gathers the rows and checks their exactness (two
    // launches where fold_in, the sampler, the gather and the key launch were four: 264 -> 254 us per step at B = 4096)
    static const bool no_fuse = getenv("D3P_VAE_RUN_UNFUSED") != nullptr;   // developer switch (A/B), read once
    const bool fused = !no_fuse && model->D % 4 == 0 && ((reinterpret_cast<uintptr_t>(X_dev) | reinterpret_cast<uintptr_t>(xb_dev)) & 15u) == 0;
    for (uint32_t t = 0; t < num_steps; ++t) {
        int rc;
        if (fused) {
            const VaeRunStep rs = {batch_key_dev, first_batch + t, X_dev, n_rows, idx_dev};
            if ((rc = vae_update_impl(stream, model, hyper, &st, xb_dev, nullptr, B, nullptr, losses_dev ? losses_dev + t : nullptr, nullptr,
                                      workspace_dev, workspace_bytes, &rs)))
                return rc;
        } else {
            if ((rc = d3p_rng_fold_in(stream, batch_key_dev, first_batch + t, step_key))) return rc;          // minibatch.py:230
            if ((rc = d3p_feistel_sample(stream, step_key, n_rows, B, idx_dev))) return rc;                   // minibatch.py:231
            if ((rc = d3p_take_rows(stream, X_dev, n_rows, (uint32_t)(model->D * sizeof(float)), idx_dev, B, nullptr, xb_dev))) return rc;
            if ((rc = d3p_dpvi_vae_update(stream, model, hyper, &st, xb_dev, nullptr, B, nullptr, losses_dev ? losses_dev + t : nullptr,
                                          nullptr, workspace_dev, workspace_bytes)))
                return rc;
        }
        st.key_slot ^= 1;
    }
    return D3P_OK;
}

// ---- the data-parallel epoch body as ONE call (examples/vae.py:227-246 with the batch sharded by position)
namespace {
struct VaeDistSide {   // per (device, caller's stream): the stream the reduces travel on and the events that order them against the step's stream
    hipStream_t cs = nullptr;
    hipEvent_t ready[2] = {nullptr, nullptr}, done = nullptr;
};
static int vae_dist_side(hipStream_t caller, VaeDistSide** out)
{
    // keyed by the caller's stream too: in-process ranks (one stream each) and host threads must not share a side stream or re-record
    // each other's events -- two ranks of one communicator on ONE side stream would wait for each other's reduce forever
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, VaeDistSide> sides;
    int dev = 0;
    D3P_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    VaeDistSide& v = sides[std::make_pair(dev, caller)];
    if (!v.cs) {
        D3P_HIP_TRY(hipStreamCreateWithFlags(&v.cs, hipStreamNonBlocking));
        for (hipEvent_t* e : {&v.ready[0], &v.ready[1], &v.done}) D3P_HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    *out = &v;
    return D3P_OK;
}
struct VaeDistStep {
    hipStream_t s;
    VaeDistSide* side;
    void* comm;
    float* sums;
    size_t split, total;   // bucket 0 = [0, split), bucket 1 = [split, total)
};
static int vae_dist_bucket_ready(void* ctx, int bucket)
{
    // bucket 0: its reduce starts on the side stream as soon as its tile sums are complete -- the second bucket's products run beside it;
    // bucket 1: behind the first on the same stream (a communicator runs one collective at a time anyway)
    VaeDistStep* d = (VaeDistStep*)ctx;
    D3P_HIP_TRY(hipEventRecord(d->side->ready[bucket], d->s));
    D3P_HIP_TRY(hipStreamWaitEvent(d->side->cs, d->side->ready[bucket], 0));
    const size_t lo = bucket == 0 ? 0 : d->split, hi = bucket == 0 ? d->split : d->total;
    if (int rc = rccl_allreduce_f32(d->comm, d->sums + lo, hi - lo, d->side->cs)) return rc;
    if (bucket == 1) {
        D3P_HIP_TRY(hipEventRecord(d->side->done, d->side->cs));
        D3P_HIP_TRY(hipStreamWaitEvent(d->s, d->side->done, 0));
    }
    return D3P_OK;
}
}  // namespace

// num_steps x [local sums of the rank's B_local examples (positions pos0 .. of the global batch of B_total) -> sum-all-reduce of the
// P + 2 fp32 sums over `comm` -> noise once + Adam, identical on every rank] on the RESIDENT shard X_local_dev, enqueued back to
// back: no host work between steps, no per-step state or key copies (the state advances in place, its key ping-pongs between the
// two slots of state->rng_key like d3p_dpvi_vae_run), the step's keys are derived once, the Gaussian-mechanism noise is drawn
// beside the latent kernel (it depends on the keys only), and apply is ONE launch behind the reduce.
// buckets = 2: the sums travel in two buckets on a second stream -- the decoder's leaves while the encoder's weight-gradient
// products still run (VaeBuckets); 1: one all-reduce on `stream` itself; 0: the library's choice (1: see below).
// comm = NULL: no collective (one rank; B_local == B_total).
int d3p_dpvi_vae_run_dist(void* stream, void* comm, void* fmesh, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                          const float* X_local_dev, const uint8_t* mask_dev, uint32_t B_local, uint32_t B_total, uint32_t pos0,
                          uint32_t num_steps, float* losses_dev, int32_t buckets, void* workspace_dev, size_t workspace_bytes)
{
    // fmesh != NULL: the step's collective is the full-mesh reduce-scatter + all-gather of d3p_fmesh.hip (one launch in the stream)
    // instead of RCCL's all-reduce
    D3P_REQUIRE(!(comm && fmesh), "d3p_dpvi_vae_run_dist: one collective, RCCL (comm) or the full mesh (fmesh), not both");
    if (int rc = vae_update_checks(model, hyper, state, workspace_dev, "d3p_dpvi_vae_run_dist")) return rc;
    D3P_REQUIRE(X_local_dev, "d3p_dpvi_vae_run_dist: null pointer");
    D3P_REQUIRE(B_local >= 1 && (uint64_t)pos0 + B_local <= B_total, "d3p_dpvi_vae_run_dist: need 1 <= B_local and pos0 + B_local <= B_total");
    D3P_REQUIRE(comm || fmesh || B_local == B_total, "d3p_dpvi_vae_run_dist: a shard of the batch needs a communicator");
    D3P_REQUIRE(buckets >= 0 && buckets <= 2, "d3p_dpvi_vae_run_dist: buckets must be 0, 1 or 2");
    if (workspace_bytes < d3p_dpvi_vae_workspace(model, B_local)) return fail(D3P_E_WORKSPACE, "d3p_dpvi_vae_run_dist: workspace too small");
    VaeWorkspace ws;
    vae_carve(model, B_local, (char*)workspace_dev, &ws);
    const VaeNet N = vae_net(model);
    hipStream_t s = (hipStream_t)stream;
    static const int env_buckets = [] { const char* e = getenv("D3P_VAE_DP_BUCKETS"); return e ? atoi(e) : 0; }();   // developer switch (A/B), read once
    // (the library's choice is ONE bucket: on one GPU the two-bucket form costs 40 us per step more -- two event hand-overs between the
    // streams, one more grouped launch and tile-sum launch -- than the 30 us of products it can put beside a reduce;
    // profiles/r05_vae_dp_loop_rank_local.jsonl.  bench.py --gpus N times both over real links.)
    if (buckets == 0 && !fmesh) buckets = (env_buckets == 1 || env_buckets == 2) ? env_buckets : 1;
    VaeDistStep step = {s, nullptr, comm, ws.sums, N.enc[0].W, (size_t)N.P + 2};
    const bool two = comm && buckets == 2 && !vae_no_group() && step.split > 0 && step.split < (size_t)N.P;
    if (two)
        if (int rc = vae_dist_side(s, &step.side)) return rc;
    const VaeBuckets bk = {step.split, vae_dist_bucket_ready, &step};
    d3p_dpsvi_state st = *state;
    // full mesh: the tile sums, the collective and the update as ONE launch (k_vae_fmesh_step); D3P_VAE_FMESH_UNFUSED=1 keeps them apart
    static const bool fm_unfused = getenv("D3P_VAE_FMESH_UNFUSED") != nullptr;   // developer switch (A/B), read once
    for (uint32_t t = 0; t < num_steps; ++t) {
        int rc;
        if (fmesh && !fm_unfused && buckets != 1) {   // (buckets = 1 with a mesh: tile sums, collective and update as three launches)
            FMesh* x = (FMesh*)fmesh;
            D3P_REQUIRE(x->n == (uint64_t)N.P + 2, "d3p_dpvi_vae_run_dist: the mesh was created for another vector length (P + 2)");
            for (int p = 0; p < x->world; ++p) D3P_REQUIRE(x->peer[p], "d3p_dpvi_vae_run_dist: the peers' inboxes are not mapped (d3p_fmesh_connect)");
            int w_splits[D3P_VAE_MAX_BLOCKS];
            bool loss_pending = false;
            // (the single-device update's local phase: the split-K partial tiles stay where they are, the noise is drawn beside the latent kernel)
            if ((rc = vae_local_sums_impl(stream, model, hyper, &st, X_local_dev, mask_dev, B_local, B_total, pos0, nullptr, ws.sums, workspace_dev,
                                          workspace_bytes, true, w_splits, nullptr, nullptr, &loss_pending)))
                return rc;
            if (loss_pending)   // (the loss sum is still per example -- the output layer's epilogue without the grouped launch: one more launch sums it)
                hipLaunchKernelGGL(k_vae_loss_n, dim3(1), dim3(256), 0, s, (const float*)ws.px_loss, mask_dev, B_local, ws.sums + N.P);
            const VaeFinalArgs f = vae_final_args(model, hyper, &st, ws, ws.sums, B_total, B_local, losses_dev ? losses_dev + t : nullptr, nullptr, w_splits,
                                                  nullptr, false);
            FMeshArgs ma;
            fmesh_next_args(x, ws.sums, &ma);
            hipLaunchKernelGGL(k_vae_fmesh_step, dim3((unsigned)x->wgs), dim3(256), 0, s, ma, f);
            if ((rc = check_launch("k_vae_fmesh_step"))) return rc;
            st.key_slot ^= 1;
            continue;
        }
        if ((rc = vae_local_sums_impl(stream, model, hyper, &st, X_local_dev, mask_dev, B_local, B_total, pos0, nullptr, ws.sums, workspace_dev,
                                      workspace_bytes, true, nullptr, nullptr, nullptr, nullptr, true, two ? &bk : nullptr)))
            return rc;
        if (comm && !two && (rc = rccl_allreduce_f32(comm, ws.sums, (size_t)N.P + 2, s))) return rc;
        if (fmesh && (rc = fmesh_enqueue_allreduce(s, fmesh, ws.sums, (uint64_t)N.P + 2))) return rc;
        if ((rc = vae_apply_impl(stream, model, hyper, &st, ws.sums, B_total, B_local, losses_dev ? losses_dev + t : nullptr, nullptr, workspace_dev,
                                 workspace_bytes, false, nullptr, nullptr, false, true)))
            return rc;
        st.key_slot ^= 1;
    }
    return D3P_OK;
}

}  // extern "C"
