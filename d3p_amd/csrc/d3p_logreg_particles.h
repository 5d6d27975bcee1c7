// Multi-particle ELBO gradients (numpyro Trace_ELBO(num_particles=K), K > 1) for the logistic-regression / Gaussian-mean
// families.  Example p's gradient is the MEAN over its K particles' gradients, taken before the joint norm and the clip
// (svi.py:310-325 clips the vmapped gradient of the mean loss); its loss is the mean of the particle losses.  Particle q draws
// its guide noise from px_particle_sample_key (d3p_logreg_kernel.h), or reads it from eps_ext laid out (B, K, D).
//
// One wavefront per example.  Per particle, two passes over the example's column pairs (c, c + half) -- the threefry pair
// layout of k_logreg_main / k_logreg_wide:
//   pass 1: eps (generated once, kept in the wavefront's LDS row), z = loc + s eps, logit x . z (Gaussian mean: the squared
//           residual norm) and the latent part of the loss                                    (svi.py:238-281)
//   pass 2: the particle's gradient entries, added to the wavefront's gradient-sum row in LDS   (svi.py:291-306)
// then the sum row times 1/K is the example's gradient.  PXG = false (clip-and-accumulate stage): joint norm -> clip factor ->
// clipped row added to the wavefront's accumulator row, and one partial row of P + 2 floats per workgroup in the layout of
// k_logreg_main's MODE 0 (consumed by k_reduce_partials / k_finalize).  PXG = true (materialising stage, d3p_logreg_px_grads_particles):
// the averaged row and loss of every batch position (zeros for masked ones).  Every lane only ever touches its own columns of the
// LDS rows, so no barrier is needed inside an example.  The row of X and the label are read from memory by every pass of every
// particle, but within a few microseconds of each other: HBM sees them once, the rest hit the caches.  No atomics: deterministic.
#pragma once
#include "d3p_logreg_kernel.h"

namespace d3p {

#define D3P_PART_MAX_BLOCKS 1024u

struct ParticleArgs {
    MainArgs a;               // X, y, idx, mask, counts, plist / n_list, eps_ext (B x K x D), pack, partials / px_* , scalars
    const uint32_t* jax_key;  // the step's jax key (2 words): particle keys are derived here (unused with eps_ext)
    uint32_t K;               // particles per example (> 1)
};

// floats of LDS per wavefront: gradient-sum row (P) | eps row (D) | accumulator row (P, clip-and-accumulate stage only)
__host__ __device__ static inline size_t particles_wave_floats(int D, bool pxg) { return (size_t)((pxg ? 2 : 4) * D + D + 3) & ~(size_t)3; }
static inline size_t particles_lds_bytes(int D, int W, bool pxg) { return ((size_t)W * particles_wave_floats(D, pxg) + 2 * W) * sizeof(float); }

// wavefronts per workgroup: 4, or fewer when the rows do not fit the CU's 160 KB of LDS (less a line for the static word of
// __syncthreads_or); 0: not even one does
#define D3P_PART_LDS_MAX (160u * 1024u - 256u)
static inline int particles_waves(int D, bool pxg)
{
    for (int W = 4; W >= 1; W >>= 1)
        if (particles_lds_bytes(D, W, pxg) <= D3P_PART_LDS_MAX) return W;
    return 0;
}

// the largest D (d + intercept) a stage runs at one wavefront per workgroup: 8178 (clip-and-accumulate), 13630 (materialising)
static inline int particles_max_latent(bool pxg)
{
    int D = (int)(D3P_PART_LDS_MAX / sizeof(float)) / (pxg ? 3 : 5) + 1;
    while (D > 0 && particles_waves(D, pxg) == 0) --D;
    return D;
}

// GLM: 0, or the family of a linear / Poisson regression instantiation (as k_logreg_main's): the link is a compile-time choice.
template <bool PXG, int GLM = 0>
__global__ void __launch_bounds__(256) k_logreg_particles(ParticleArgs pa)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MainArgs& a = pa.a;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = (int)(blockDim.x >> 6);
    const int D = a.D, half = a.half, P = 2 * D, d = a.d;
    const uint32_t K = pa.K;
    const float invK = 1.0f / (float)K;
    float* grow = lds + (size_t)wave * particles_wave_floats(D, PXG);  // [g (D) | h (D)]: sum over the particles
    float* erow = grow + P;                                            // eps of the current particle
    float* acc = erow + D;                                             // clipped rows of this wavefront (!PXG)
    float* tail = lds + (size_t)W * particles_wave_floats(D, PXG);
    const float* pk = a.pack;  // [loc | s | sg | q | lc] x D
    const bool eps_from_mem = a.eps_ext != nullptr;
    const bool gauss = !GLM && a.family == D3P_FAMILY_GAUSS_MEAN;
    constexpr int glm_family = GLM ? GLM : D3P_FAMILY_LOGREG;
    const uint32_t j0 = eps_from_mem ? 0u : pa.jax_key[0], j1 = eps_from_mem ? 0u : pa.jax_key[1];
    if (!PXG) {
        for (int c = lane; c < P; c += 64) acc[c] = 0.f;
        __syncthreads();
    }
    const uint32_t n_valid = a.counts ? a.counts[1] : a.B;
    const uint32_t n_items = a.plist ? *a.n_list : a.B;
    const uint32_t total_waves = gridDim.x * (uint32_t)W;
    float loss_acc = 0.f, n_acc = 0.f;
    // (materialising stage) a parameter that is not finite makes a masked example's loss * mask NaN (svi.py:281), as in k_logreg_wide
    float skipped = 0.f;
    if (PXG) {
        int p_bad = 0;
        for (int c = threadIdx.x; c < 5 * D; c += blockDim.x) p_bad |= !(fabsf(pk[c]) <= 3.402823466e38f);
        if (__syncthreads_or(p_bad)) skipped = __builtin_nanf("");
    }
    auto col_c1 = [&](int c) { return (a.icpt && c == d) ? a.c1_b : a.c1_w; };
    auto col_hz = [&](int c) { return (a.icpt && c == d) ? a.hz_b : a.hz_w; };

    for (uint32_t item = blockIdx.x * (uint32_t)W + (uint32_t)wave; item < n_items; item += total_waves) {
        const uint32_t pp = a.plist ? a.plist[item] : item;
        const uint32_t row_g = a.idx ? a.idx[pp] : pp;
        const bool valid = (pp < n_valid) && (a.mask ? a.mask[pp] != 0 : true);
        const bool own = (uint64_t)row_g >= a.row_lo && (uint64_t)row_g < a.row_hi;
        if (!(valid && own)) {  // wave-uniform
            if (PXG) {  // loss * mask => zero loss and gradient (svi.py:281)
                float* gr = a.px_grads + (size_t)pp * P;
                for (int c = lane; c < P; c += 64) gr[c] = skipped;
                if (lane == 0) a.px_loss[pp] = skipped;
            }
            continue;
        }
        const size_t row = (size_t)((uint64_t)row_g - a.row_lo);
        const float* xrow = a.X + row * (size_t)d;
        const float yv = a.y ? a.y[row] : 0.f;
        const float label_c = glm_label_const(glm_family, yv, a.ll_const);  // (once per example: no particle's parameters reach it)
        auto feat = [&](int c) { return c < d ? xrow[c] : 1.0f; };  // column d = intercept
        float Lsum = 0.f;
        for (uint32_t q = 0; q < K; ++q) {
            uint32_t k0 = 0u, k1 = 0u;
            if (!eps_from_mem) px_particle_sample_key(j0, j1, a.B, pp, K, q, k0, k1);
            const float* er = eps_from_mem ? a.eps_ext + ((size_t)pp * K + q) * D : nullptr;

            // ---- pass 1: eps, logit and the latent part of the loss
            float tp = 0.f, lp = 0.f;
            for (int c0 = lane; c0 < half; c0 += 64) {
                const int c1 = c0 + half;
                const bool ok1 = c1 < D;
                float e0, e1;
                if (eps_from_mem) {
                    e0 = er[c0];
                    e1 = ok1 ? er[c1] : 0.f;
                } else {
                    uint32_t b0, b1;
                    threefry2x32(k0, k1, (uint32_t)c0, ok1 ? (uint32_t)c1 : 0u, b0, b1);
                    // (bits_to_normal, not the wave-uniform form: the lanes of the last pairs of a row run this loop alone, and it is
                    // the arithmetic of d3p_px_eps_sites_particles, so on-chip draws and that stream agree bit for bit)
                    e0 = bits_to_normal(b0);
                    e1 = ok1 ? bits_to_normal(b1) : 0.f;
                }
                erow[c0] = e0;
                if (ok1) erow[c1] = e1;
                const float z0 = __fmaf_rn(pk[D + c0], e0, pk[c0]);
                float x0 = feat(c0);
                if (gauss) x0 -= z0;  // residuals take the place of the features: dloglik/dz = (x - z) / sigma^2
                tp = __fmaf_rn(x0, gauss ? x0 : z0, tp);
                lp += __fmaf_rn(col_hz(c0) * z0, z0, __fmaf_rn(-0.5f * e0, e0, pk[4 * D + c0]));
                if (ok1) {
                    const float z1 = __fmaf_rn(pk[D + c1], e1, pk[c1]);
                    float x1 = feat(c1);
                    if (gauss) x1 -= z1;
                    tp = __fmaf_rn(x1, gauss ? x1 : z1, tp);
                    lp += __fmaf_rn(col_hz(c1) * z1, z1, __fmaf_rn(-0.5f * e1, e1, pk[4 * D + c1]));
                }
            }
            const float t = wave_sum(tp);
            lp = wave_sum(lp);
            float A, loglik;
            if (gauss) {
                A = 2.0f * a.A_scale * a.nh_inv_var;
                loglik = __fmaf_rn(a.nh_inv_var, t, -a.ll_const);
            } else {  // the regression families' link
                glm_link(glm_family, t, yv, a.A_scale, a.nh_inv_var, label_c, A, loglik);
            }
            Lsum += a.inv_obs * (lp - a.lik_scale * loglik);  // svi.py:278-281

            // ---- pass 2: the particle's gradient entries into the sum row
            auto grad_col = [&](int c) {
                const float e = erow[c];
                const float z = __fmaf_rn(pk[D + c], e, pk[c]);
                const float x = gauss ? feat(c) - z : feat(c);
                const float g = __fmaf_rn(col_c1(c), z, A * x);
                const float h = __fmaf_rn(g * e, pk[2 * D + c], -pk[3 * D + c]);
                grow[c] = q == 0 ? g : grow[c] + g;
                grow[D + c] = q == 0 ? h : grow[D + c] + h;
            };
            for (int c0 = lane; c0 < half; c0 += 64) {
                grad_col(c0);
                if (c0 + half < D) grad_col(c0 + half);
            }
        }
        const float L = Lsum * invK;

        if (PXG) {
            float* gr = a.px_grads + (size_t)pp * P;
            for (int c0 = lane; c0 < half; c0 += 64) {
                for (int c = c0; c < D; c += half) {
                    gr[c] = grow[c] * invK;
                    gr[D + c] = grow[D + c] * invK;
                }
            }
            if (lane == 0) a.px_loss[pp] = L * a.obs_scale * a.meta[1];  // svi.py:306
            continue;
        }

        // ---- joint norm of the averaged row, clip factor, clipped row into the accumulator (svi.py:68-124, :343-346)
        float n2 = 0.f;
        for (int c0 = lane; c0 < half; c0 += 64) {
            for (int c = c0; c < D; c += half) {
                const float g = grow[c] * invK, h = grow[D + c] * invK;
                n2 = __fmaf_rn(g, g, n2);
                n2 = __fmaf_rn(h, h, n2);
            }
        }
        n2 = wave_sum(n2);
        const float cf = fminf(1.0f, a.clip * __builtin_amdgcn_rsqf(n2));  // svi.py:121-122
        for (int c0 = lane; c0 < half; c0 += 64) {
            for (int c = c0; c < D; c += half) {
                acc[c] = __fmaf_rn(cf, grow[c] * invK, acc[c]);
                acc[D + c] = __fmaf_rn(cf, grow[D + c] * invK, acc[D + c]);
            }
        }
        loss_acc += L;
        n_acc += 1.0f;
    }

    if (PXG) return;
    if (lane == 0) { tail[2 * wave] = loss_acc; tail[2 * wave + 1] = n_acc; }
    __syncthreads();
    const size_t stride = particles_wave_floats(D, false);
    float* out = a.partials + (size_t)blockIdx.x * (P + 2);
    for (int c = threadIdx.x; c < P; c += blockDim.x) {
        float s = 0.f;
        for (int w = 0; w < W; ++w) s += lds[(size_t)w * stride + 3 * D + c];
        out[c] = s;
    }
    // (workgroup 0: a step parameter that is not finite makes the loss NaN even when no example is valid, as in k_logreg_main)
    int p_bad = 0;
    if (blockIdx.x == 0) {
        for (int c = threadIdx.x; c < 5 * D; c += blockDim.x) p_bad |= !(fabsf(pk[c]) <= 3.402823466e38f);
        p_bad = __syncthreads_or(p_bad);
    }
    if (threadIdx.x < 2) {
        float s = 0.f;
        for (int w = 0; w < W; ++w) s += tail[2 * w + threadIdx.x];
        if (threadIdx.x == 0 && p_bad) s = __builtin_nanf("");
        out[P + threadIdx.x] = s;
    }
}

// Workgroups of either form for `items` examples: W wavefronts each (particles_waves), at most D3P_PART_MAX_BLOCKS (waves loop
// over further examples).  The clip-and-accumulate stage writes one partial row per workgroup: k_finalize adds this many.
static inline uint32_t particles_blocks(int D, bool pxg, uint64_t items)
{
    const int W = particles_waves(D, pxg);
    uint64_t blocks = W ? (items + (uint64_t)W - 1) / (uint64_t)W : 1;
    if (blocks < 1) blocks = 1;
    return (uint32_t)(blocks > D3P_PART_MAX_BLOCKS ? D3P_PART_MAX_BLOCKS : blocks);
}

template <bool PXG, int GLM = 0>
static int launch_particles(hipStream_t s, const ParticleArgs& pa, uint32_t blocks, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr)
{
    if (!GLM && pa.a.family == D3P_FAMILY_LINREG) return launch_particles<PXG, D3P_FAMILY_LINREG>(s, pa, blocks, e0, e1);
    if (!GLM && pa.a.family == D3P_FAMILY_POISSON) return launch_particles<PXG, D3P_FAMILY_POISSON>(s, pa, blocks, e0, e1);
    const int D = pa.a.D;
    const int W = particles_waves(D, PXG);
    if (W == 0)
        return fail(D3P_E_UNSUPPORTED, "k_logreg_particles: rows of %d latent columns do not fit the LDS (at most %d)", D,
                    particles_max_latent(PXG));
    if (pa.K < 2u) return fail(D3P_E_INVALID_ARG, "k_logreg_particles: K = 1 runs on the single-particle kernels");
    const size_t lds = particles_lds_bytes(D, W, PXG);
    // (the attribute is per function and device: set on every launch that needs it -- only rows of more than ~1600 columns do)
    if (lds > 64u * 1024u && hipFuncSetAttribute(reinterpret_cast<const void*>(k_logreg_particles<PXG, GLM>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)D3P_PART_LDS_MAX) != hipSuccess) {
        (void)hipGetLastError();
        return fail(D3P_E_HIP, "k_logreg_particles: hipFuncSetAttribute(MaxDynamicSharedMemorySize, %zu) failed", lds);
    }
    if (e0)
        hipExtLaunchKernelGGL((k_logreg_particles<PXG, GLM>), dim3(blocks), dim3(64 * W), lds, s, e0, e1, 0, pa);
    else
        hipLaunchKernelGGL((k_logreg_particles<PXG, GLM>), dim3(blocks), dim3(64 * W), lds, s, pa);
    return check_launch("k_logreg_particles");
}

}  // namespace d3p
