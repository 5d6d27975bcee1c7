// Clipping diagnostics (d3p_amd/clipping.py, include/d3p_hip.h): the per-example gradient NORMS of the regression
// families without the rows x P tensor, d3p_logreg_grad_norms, and a model-free profile of a vector of norms, d3p_norm_profile.
//
// k_grad_norms.  norms[r] is the float32 L2 norm of the row d3p_logreg_px_grads writes for example r (the arithmetic of
// k_logreg_main's MODE 1, statement for statement: the same fused multiply-adds, glm_link, guide_scale through k_pack), summed over
// the lanes in wave_sum's fixed order.  One wavefront per row, four per workgroup, rows strided over the grid; the packed columns
// (loc | s | sg | q | lc: 5 D floats, <= 40 KiB) are copied to LDS once per workgroup.  Lane l owns the column pairs
// (c, c + half), c = 64 k + l, k < NC, half = ceil(D / 2): one threefry call of the example's sample key per pair, both words used
// (jax's iota layout), and consecutive lanes read consecutive floats of the row.  x and eps of the lane's <= 2 NC = 34 columns stay in
// registers over two sweeps: z = loc + s eps and the wave sum of x z, the link, then the two gradient entries per column squared and
// summed.  X is read once; nothing of size rows x D is written.  NC (1, 2, 3, 5, 9, 13, 17) and the link are compile-time choices.
// The example's key is px_sample_key(jax_key, B_total, pos0 + r): lane l derives the key of the wave's (64 i + l)-th row once per 64
// rows, the wave reads it back by lane -- 6 threefry calls per 64 rows per lane instead of 6 per row.
// No atomics, no clamps: a sum of squares beyond float32 gives inf, exp(t) = inf a non-finite norm.
//
// k_norm_pass / k_norm_final.  One pass over the vector per 8-bit digit of an order-preserving uint32 key (key_f32 of
// d3p_colreduce.h), most significant first, with all 2 Q wanted ranks in flight: ranks that still share a prefix share
// one histogram.  Workgroup b owns strip b of the vector (the strip count is a function of n alone); it builds its histograms in LDS
// with integer atomics and adds them to the launch's with 64-bit integer atomics -- order-independent, hence deterministic.  The
// prefix of a pass is derived from the previous pass's histogram by every workgroup at its start.  Pass 0 also forms the strip's
// counts and float64 sums (a thread's elements in index order, the lanes by an xor butterfly, the four waves in order); k_norm_final
// merges the strips in strip order, finishes the selection and interpolates in float64, rounding to float32 once.  Only NON-finite
// values are left out of the selection; no float atomics anywhere.
#include "d3p_colreduce.h"
#include "d3p_logreg_kernel.h"

#pragma clang fp contract(off)

namespace d3p {

#define D3P_GN_WAVES 4
#define D3P_GN_MAX_D 2048
#define D3P_GN_MAX_BLOCKS 2048u

struct GradNormArgs {
    const float* X;
    const float* y;
    const float* eps;          // nullable: rows x D
    const uint32_t* jax_key;   // read where eps is null
    const float* pack;         // 5 x D
    float* norms;
    float* px_loss;            // nullable
    uint32_t B_total, pos0, rows;
    int d, D, half, icpt;
    float A_scale, c1_w, c1_b, hz_w, hz_b, inv_obs, lik_scale, obs_scale, nh_inv_var, ll_const;
};

// Registers (hipcc 7.2, gfx950; tools/kernel_resources.py): no scratch in any instantiation, DESIGN.md 4n has the table.
template <int NC, int GLM>
__global__ void __launch_bounds__(64 * D3P_GN_WAVES) k_grad_norms(GradNormArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float gn_pk[];   // loc | s | sg | q | lc
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = a.d, D = a.D, half = a.half;
    for (int i = threadIdx.x; i < 5 * D; i += 64 * D3P_GN_WAVES) gn_pk[i] = a.pack[i];
    __syncthreads();   // (the only barrier: from here on every wave runs alone)
    const float* pk = gn_pk;

    int c0[NC], c1[NC];
    bool ok0[NC], ok1[NC];
#pragma unroll
    for (int n = 0; n < NC; ++n) {
        c0[n] = 64 * n + lane;
        c1[n] = c0[n] + half;
        ok0[n] = c0[n] < half;
        ok1[n] = ok0[n] && c1[n] < D;
    }
    const bool onchip = a.eps == nullptr;
    uint32_t j0 = 0u, j1 = 0u;
    if (onchip) { j0 = a.jax_key[0]; j1 = a.jax_key[1]; }
    const uint64_t rows = a.rows, stride = (uint64_t)gridDim.x * D3P_GN_WAVES;
    uint32_t kk0 = 0u, kk1 = 0u;   // lane l: the sample key of the row this wave reaches l iterations after the last refill
    uint32_t it = 0u;
    for (uint64_t r = (uint64_t)blockIdx.x * D3P_GN_WAVES + wave; r < rows; r += stride, ++it) {
        if (onchip && (it & 63u) == 0u) {
            uint64_t rl = r + (uint64_t)lane * stride;
            rl = rl < rows ? rl : rows - 1u;   // (a lane past the end derives a key nobody reads)
            px_sample_key(j0, j1, a.B_total, a.pos0 + (uint32_t)rl, kk0, kk1);
        }
        const float* xrow = a.X + (size_t)r * (size_t)d;
        float x0[NC], x1[NC], e0[NC], e1[NC];
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            x0[n] = ok0[n] ? (c0[n] < d ? xrow[c0[n]] : 1.0f) : 0.f;   // column d = intercept
            x1[n] = ok1[n] ? (c1[n] < d ? xrow[c1[n]] : 1.0f) : 0.f;
        }
        const float y = a.y[r];
        if (!onchip) {
            const float* er = a.eps + (size_t)r * (size_t)D;
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                e0[n] = ok0[n] ? er[c0[n]] : 0.f;
                e1[n] = ok1[n] ? er[c1[n]] : 0.f;
            }
        } else {
            const int src = __builtin_amdgcn_readfirstlane((int)(it & 63u));
            const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)kk0, src), k1 = (uint32_t)__builtin_amdgcn_readlane((int)kk1, src);
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                uint32_t b0, b1;
                threefry2x32(k0, k1, (uint32_t)c0[n], ok1[n] ? (uint32_t)c1[n] : 0u, b0, b1);
                const float v0 = bits_to_normal_wu(b0), v1 = bits_to_normal_wu(b1);
                e0[n] = ok0[n] ? v0 : 0.f;
                e1[n] = ok1[n] ? v1 : 0.f;
            }
        }
        // ---- sweep 1: z = loc + s eps, t = x . z (the intercept's x is 1)
        float tp = 0.f;
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const float l0 = ok0[n] ? pk[c0[n]] : 0.f, l1 = ok1[n] ? pk[c1[n]] : 0.f;
            const float s0 = ok0[n] ? pk[D + c0[n]] : 0.f, s1 = ok1[n] ? pk[D + c1[n]] : 0.f;
            tp = __fmaf_rn(x0[n], __fmaf_rn(s0, e0[n], l0), tp);
            tp = __fmaf_rn(x1[n], __fmaf_rn(s1, e1[n], l1), tp);
        }
        const float t = wave_sum(tp);
        float A, loglik;
        glm_link(GLM, t, y, a.A_scale, a.nh_inv_var, glm_label_const(GLM, y, a.ll_const), A, loglik);
        // ---- sweep 2: the row's two entries per column, squared and summed; the latent part of the loss
        float n2 = 0.f, lp = 0.f;
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            const bool ic0 = a.icpt && c0[n] == d, ic1 = a.icpt && c1[n] == d;
            const float l0 = ok0[n] ? pk[c0[n]] : 0.f, l1 = ok1[n] ? pk[c1[n]] : 0.f;
            const float s0 = ok0[n] ? pk[D + c0[n]] : 0.f, s1 = ok1[n] ? pk[D + c1[n]] : 0.f;
            const float sg0 = ok0[n] ? pk[2 * D + c0[n]] : 0.f, sg1 = ok1[n] ? pk[2 * D + c1[n]] : 0.f;
            const float q0 = ok0[n] ? pk[3 * D + c0[n]] : 0.f, q1 = ok1[n] ? pk[3 * D + c1[n]] : 0.f;
            const float lc0 = ok0[n] ? pk[4 * D + c0[n]] : 0.f, lc1 = ok1[n] ? pk[4 * D + c1[n]] : 0.f;
            const float z0 = __fmaf_rn(s0, e0[n], l0), z1 = __fmaf_rn(s1, e1[n], l1);
            const float g0 = __fmaf_rn(ic0 ? a.c1_b : a.c1_w, z0, A * x0[n]);
            const float g1 = __fmaf_rn(ic1 ? a.c1_b : a.c1_w, z1, A * x1[n]);
            const float h0 = __fmaf_rn(g0 * e0[n], sg0, -q0);
            const float h1 = __fmaf_rn(g1 * e1[n], sg1, -q1);
            n2 = __fmaf_rn(g0, g0, n2);
            n2 = __fmaf_rn(h0, h0, n2);
            n2 = __fmaf_rn(g1, g1, n2);
            n2 = __fmaf_rn(h1, h1, n2);
            lp += __fmaf_rn((ic0 ? a.hz_b : a.hz_w) * z0, z0, __fmaf_rn(-0.5f * e0[n], e0[n], lc0));
            lp += __fmaf_rn((ic1 ? a.hz_b : a.hz_w) * z1, z1, __fmaf_rn(-0.5f * e1[n], e1[n], lc1));
        }
        n2 = wave_sum(n2);
        if (lane == 0) a.norms[r] = __fsqrt_rn(n2);
        if (a.px_loss) {   // (uniform) L_i = inv_obs ((logq - logp) - lik_scale loglik), times obs_scale and the factor B / n = 1
            lp = wave_sum(lp);
            const float L = a.inv_obs * (lp - a.lik_scale * loglik);
            if (lane == 0) a.px_loss[r] = L * a.obs_scale;
        }
    }
}

// ---- the profile of a vector of norms ------------------------------------------------------------------------------------------------
#define D3P_NP_MAX 8                  // thresholds and probabilities per call
#define D3P_NP_RANKS (2 * D3P_NP_MAX)
#define D3P_NP_MAX_STRIPS 1024u
#define D3P_NP_STRIP_MIN 4096u        // elements per strip before the strip count reaches its maximum
#define D3P_NP_HSTRIDE 257            // 256 bins + 1 (the 16 scanning threads fall on different banks)
#define D3P_NP_PART_WORDS 21          // n_finite | n_nonfinite | sum | sum of squares | max key | n_clipped[8] | clip-factor sums[8]
#define D3P_NP_OUT_WORDS 29           // n_finite | n_nonfinite | mean | mean of squares | max | n_clipped[8] | mean_clip_factor[8] | quantiles[8]
#define D3P_NP_MAX_N (1ull << 40)

struct NpState {      // one wanted rank after a pass
    uint32_t prefix;  // the digits found so far
    uint32_t valid;   // 0: the rank lies beyond the finite values
    uint32_t slot;    // the smallest rank index with the same prefix: the histogram both count in
    uint32_t pad;
    unsigned long long rank;   // 1-based, among the values with this prefix
};

struct NormProfArgs {
    const uint32_t* v;
    unsigned long long n, strip_len;
    uint32_t m, Q, R;
    float thr[D3P_NP_MAX];
    unsigned long long lo[D3P_NP_MAX];
    double g[D3P_NP_MAX];
    unsigned long long* hist;    // [4][16][256]
    NpState* state;              // [4][16]: state[p] is what pass p counts with
    unsigned long long* parts;   // strips x 21
    unsigned long long* out;     // 29 words
};

struct NpShared {
    unsigned long long prev[D3P_NP_RANKS * D3P_NP_HSTRIDE];   // the previous pass's histograms; afterwards this pass's (uint32)
    NpState st[D3P_NP_RANKS];
    uint32_t act_prefix[D3P_NP_RANKS], act_slot[D3P_NP_RANKS], n_act;
    unsigned long long red[4][D3P_NP_PART_WORDS];
};

// The state pass P (1 .. 4) counts with, from pass P - 1's state and histograms: every thread of the workgroup calls it; on return
// sh.st holds the states (4: the finished keys).  Workgroup 0 of a pass kernel stores them for the next one.
template <int P>
__device__ inline void np_derive(const NormProfArgs& a, NpShared& sh)
{
    const int t = threadIdx.x;
    const uint32_t R = a.R;
    const NpState* before = a.state + (size_t)(P - 1) * D3P_NP_RANKS;
    for (uint32_t j = 0; j < R; ++j) {   // pass 0 has one histogram for all ranks
        const uint32_t row = P == 1 ? 0u : before[j].slot;
        sh.prev[j * D3P_NP_HSTRIDE + t] = a.hist[((size_t)(P - 1) * D3P_NP_RANKS + row) * 256 + t];
    }
    __syncthreads();
    if ((uint32_t)t < R) {
        const NpState b = before[t];
        const unsigned long long* h = sh.prev + (size_t)t * D3P_NP_HSTRIDE;
        unsigned long long cum = 0ull, rank = 1ull;
        uint32_t bin = 0u;
        bool found = false;
        for (int j = 0; j < 256; ++j) {
            const unsigned long long cnt = h[j];
            if (!found && cum + cnt >= b.rank) { found = true; bin = (uint32_t)j; rank = b.rank - cum; }
            cum += cnt;
        }
        NpState s;
        s.prefix = (b.prefix << 8) | bin;
        s.valid = (b.valid && found) ? 1u : 0u;
        s.slot = (uint32_t)t;
        s.pad = 0u;
        s.rank = rank;
        sh.st[t] = s;
    }
    __syncthreads();
    if (t == 0) {   // ranks that share a prefix share the first one's histogram
        uint32_t n_act = 0u;
        for (uint32_t j = 0; j < R; ++j) {
            if (!sh.st[j].valid) continue;
            uint32_t slot = j;
            for (uint32_t i = 0; i < j; ++i)
                if (sh.st[i].valid && sh.st[i].prefix == sh.st[j].prefix) { slot = i; break; }
            sh.st[j].slot = slot;
            if (slot == j) { sh.act_prefix[n_act] = sh.st[j].prefix; sh.act_slot[n_act] = j; ++n_act; }
        }
        sh.n_act = n_act;
    }
    __syncthreads();
}

template <class T>
__device__ inline T np_wave_add(T v)   // xor butterfly: every lane ends with the same bits
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int P>
__global__ void __launch_bounds__(256) k_norm_pass(NormProfArgs a)
{
    __shared__ NpShared sh;
    const int t = threadIdx.x;
    uint32_t* h = reinterpret_cast<uint32_t*>(sh.prev);   // [16][256] once the previous histograms have been read
    if (P == 0) {
        if (blockIdx.x == 0 && (uint32_t)t < a.R) {
            NpState s;
            s.prefix = 0u; s.valid = 1u; s.slot = 0u; s.pad = 0u;
            s.rank = a.lo[t >> 1] + 1ull + ((t & 1) && a.g[t >> 1] != 0.0 ? 1ull : 0ull);   // rank 2 q: a, 2 q + 1: b (= a where g == 0)
            a.state[t] = s;
        }
    } else {
        np_derive<P>(a, sh);
        if (blockIdx.x == 0 && (uint32_t)t < a.R) a.state[(size_t)P * D3P_NP_RANKS + t] = sh.st[t];
        __syncthreads();   // (the previous histograms have been read by the scanning threads: their bytes are free)
    }
    const uint32_t n_act = P == 0 ? 1u : sh.n_act;
    const uint32_t n_hist = P == 0 ? 256u : a.R * 256u;
    for (uint32_t i = t; i < n_hist; i += 256) h[i] = 0u;
    __syncthreads();

    const unsigned long long lo = (unsigned long long)blockIdx.x * a.strip_len;
    unsigned long long hi = lo + a.strip_len;
    hi = hi < a.n ? hi : a.n;
    unsigned long long nf = 0ull, nnf = 0ull, ncl[D3P_NP_MAX];
    double sum = 0.0, sq = 0.0, cf[D3P_NP_MAX];
    uint32_t mx = 0u;   // (the key of a finite value is never 0)
#pragma unroll
    for (int k = 0; k < D3P_NP_MAX; ++k) { ncl[k] = 0ull; cf[k] = 0.0; }
    for (unsigned long long i = lo + (unsigned)t; i < hi; i += 256) {
        const uint32_t u = a.v[i];
        const bool fin = word_is_finite(u);
        const uint32_t key = key_f32(u);
        if (P == 0) {
            const float x = __uint_as_float(u);
            if (fin) {
                const double xd = (double)x;
                ++nf;
                sum += xd;
                sq += xd * xd;
                mx = key > mx ? key : mx;
                atomicAdd(&h[key >> 24], 1u);
            } else {
                ++nnf;
            }
#pragma unroll
            for (int k = 0; k < D3P_NP_MAX; ++k) {
                if ((uint32_t)k < a.m) {
                    const float c = a.thr[k];
                    if (!fin) ++ncl[k];                     // a non-finite row is clipped to 0
                    else if (x > c) { ++ncl[k]; cf[k] += (double)c / (double)x; }
                    else cf[k] += 1.0;                      // min(1, C / norm) = 1 (a zero norm included)
                }
            }
        } else if (fin) {
            const uint32_t top = key >> (32 - 8 * P), digit = (key >> (24 - 8 * P)) & 255u;
            for (uint32_t q = 0; q < n_act; ++q)
                if (top == sh.act_prefix[q]) atomicAdd(&h[sh.act_slot[q] * 256u + digit], 1u);
        }
    }
    __syncthreads();
    unsigned long long* gh = a.hist + (size_t)P * D3P_NP_RANKS * 256;
    for (uint32_t i = t; i < n_hist; i += 256) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&gh[i], (unsigned long long)c);
    }
    if (P == 0) {
        const int lane = t & 63, wave = t >> 6;
        unsigned long long w[D3P_NP_PART_WORDS];
        w[0] = np_wave_add(nf);
        w[1] = np_wave_add(nnf);
        w[2] = (unsigned long long)__double_as_longlong(np_wave_add(sum));
        w[3] = (unsigned long long)__double_as_longlong(np_wave_add(sq));
        uint32_t m2 = mx;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t other = __shfl_xor(m2, o, 64); m2 = other > m2 ? other : m2; }
        w[4] = m2;
#pragma unroll
        for (int k = 0; k < D3P_NP_MAX; ++k) {
            w[5 + k] = np_wave_add(ncl[k]);
            w[13 + k] = (unsigned long long)__double_as_longlong(np_wave_add(cf[k]));
        }
        if (lane == 0)
#pragma unroll
            for (int k = 0; k < D3P_NP_PART_WORDS; ++k) sh.red[wave][k] = w[k];
        __syncthreads();
        if (t < D3P_NP_PART_WORDS) {   // the four waves in order
            const bool is_f64 = t == 2 || t == 3 || t >= 13;
            unsigned long long r = sh.red[0][t];
            for (int q = 1; q < 4; ++q) {
                const unsigned long long o = sh.red[q][t];
                if (is_f64) r = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)r) + __longlong_as_double((long long)o));
                else if (t == 4) r = o > r ? o : r;
                else r += o;
            }
            a.parts[(size_t)blockIdx.x * D3P_NP_PART_WORDS + t] = r;
        }
    }
}

__global__ void __launch_bounds__(256) k_norm_final(NormProfArgs a, uint32_t strips)
{
    __shared__ NpShared sh;
    __shared__ unsigned long long tot[D3P_NP_PART_WORDS];
    const int t = threadIdx.x;
    if (a.R) np_derive<4>(a, sh);
    if (t < D3P_NP_PART_WORDS) {   // the strips in strip order
        const bool is_f64 = t == 2 || t == 3 || t >= 13;
        unsigned long long r = a.parts[t];
        for (uint32_t s = 1; s < strips; ++s) {
            const unsigned long long o = a.parts[(size_t)s * D3P_NP_PART_WORDS + t];
            if (is_f64) r = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)r) + __longlong_as_double((long long)o));
            else if (t == 4) r = o > r ? o : r;
            else r += o;
        }
        tot[t] = r;
    }
    __syncthreads();
    const unsigned long long nf = tot[0];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    auto put = [&](int i, double v) { a.out[i] = (unsigned long long)__double_as_longlong(v); };
    if (t == 0) {
        a.out[0] = nf;
        a.out[1] = tot[1];
        put(2, nf ? __longlong_as_double((long long)tot[2]) / (double)nf : nan);
        put(3, nf ? __longlong_as_double((long long)tot[3]) / (double)nf : nan);
        put(4, nf ? (double)f32_of_key((uint32_t)tot[4]) : nan);
    }
    if (t < D3P_NP_MAX) {
        a.out[5 + t] = (uint32_t)t < a.m ? tot[5 + t] : 0ull;
        put(13 + t, (uint32_t)t < a.m ? __longlong_as_double((long long)tot[13 + t]) / (double)a.n : 0.0);
        double res = nan;
        if ((uint32_t)t < a.Q && sh.st[2 * t].valid && sh.st[2 * t + 1].valid) {
            const double va = (double)f32_of_key(sh.st[2 * t].prefix), vb = (double)f32_of_key(sh.st[2 * t + 1].prefix);
            res = (double)(float)lerp_linear(va, vb, a.g[t]);   // rounded to float32 once
        }
        put(21 + t, (uint32_t)t < a.Q ? res : 0.0);
    }
}

static uint32_t np_strips(uint64_t n)
{
    const uint64_t s = (n + D3P_NP_STRIP_MIN - 1) / D3P_NP_STRIP_MIN;
    return (uint32_t)(s > D3P_NP_MAX_STRIPS ? D3P_NP_MAX_STRIPS : s < 1 ? 1 : s);
}
static const size_t NP_HIST_BYTES = (size_t)4 * D3P_NP_RANKS * 256 * 8;
static const size_t NP_STATE_BYTES = (size_t)4 * D3P_NP_RANKS * sizeof(NpState);

static size_t gn_ws_bytes(const d3p_logreg_model* m) { return align_up(5 * ((size_t)m->d + (m->intercept ? 1 : 0)) * sizeof(float), 256); }

template <int GLM>
static void gn_launch(hipStream_t s, int nc, dim3 grid, size_t lds, const GradNormArgs& a)
{
    const dim3 block(64 * D3P_GN_WAVES);
    if (nc <= 1) hipLaunchKernelGGL((k_grad_norms<1, GLM>), grid, block, lds, s, a);
    else if (nc <= 2) hipLaunchKernelGGL((k_grad_norms<2, GLM>), grid, block, lds, s, a);
    else if (nc <= 3) hipLaunchKernelGGL((k_grad_norms<3, GLM>), grid, block, lds, s, a);
    else if (nc <= 5) hipLaunchKernelGGL((k_grad_norms<5, GLM>), grid, block, lds, s, a);
    else if (nc <= 9) hipLaunchKernelGGL((k_grad_norms<9, GLM>), grid, block, lds, s, a);
    else if (nc <= 13) hipLaunchKernelGGL((k_grad_norms<13, GLM>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_grad_norms<17, GLM>), grid, block, lds, s, a);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

size_t d3p_logreg_grad_norms_workspace(const d3p_logreg_model* model, uint32_t rows)
{
    (void)rows;   // (the packed columns only: nothing of the workspace grows with the rows)
    return model && model->d >= 1 ? gn_ws_bytes(model) : 0;
}

int d3p_logreg_grad_norms(void* stream, const d3p_logreg_model* model, const float* params_dev, const float* X_dev, const float* y_dev,
                          uint32_t B_total, uint32_t pos0, uint32_t rows, const float* eps_dev, const uint32_t* jax_key_dev, float* norms_dev,
                          float* px_loss_dev, void* workspace_dev, size_t workspace_bytes)
{
    const char* what = "d3p_logreg_grad_norms";
    if (!model) return fail(D3P_E_INVALID_ARG, "%s: null model", what);
    if (model->family == D3P_FAMILY_GAUSS_MEAN)
        return fail(D3P_E_UNSUPPORTED, "%s: the Gaussian-mean family is not built (D3P_FAMILY_LOGREG, _LINREG, _POISSON)", what);
    if (int rc = validate_model(model, y_dev, what)) return rc;   // D3P_GUIDE_EXP_SITES: D3P_E_UNSUPPORTED
    if (model->d > D3P_GN_MAX_D)
        return fail(D3P_E_UNSUPPORTED, "%s: d = %d exceeds the kernel's limit d <= %d", what, model->d, D3P_GN_MAX_D);
    if ((uint64_t)pos0 + rows > B_total)
        return fail(D3P_E_UNSUPPORTED, "%s: pos0 + rows = %llu exceeds B_total = %u", what, (unsigned long long)pos0 + rows, B_total);
    if (rows == 0) return D3P_OK;
    D3P_REQUIRE(params_dev && X_dev && norms_dev && workspace_dev, "d3p_logreg_grad_norms: null pointer");
    D3P_REQUIRE(eps_dev || jax_key_dev, "d3p_logreg_grad_norms: either eps_dev or jax_key_dev must be given");
    if (workspace_bytes < gn_ws_bytes(model))
        return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace_bytes, gn_ws_bytes(model));
    hipStream_t s = (hipStream_t)stream;
    MainArgs ma;
    memset(&ma, 0, sizeof(ma));
    fill_model_scalars(model, &ma);
    const int D = ma.D;
    float* pack = (float*)workspace_dev;
    hipLaunchKernelGGL(k_pack, dim3(cdiv(D, 256)), dim3(256), 0, s, *model, params_dev, pack);
    GradNormArgs a;
    a.X = X_dev; a.y = y_dev; a.eps = eps_dev; a.jax_key = jax_key_dev; a.pack = pack; a.norms = norms_dev; a.px_loss = px_loss_dev;
    a.B_total = B_total; a.pos0 = pos0; a.rows = rows;
    a.d = ma.d; a.D = D; a.half = ma.half; a.icpt = ma.icpt;
    a.A_scale = ma.A_scale; a.c1_w = ma.c1_w; a.c1_b = ma.c1_b; a.hz_w = ma.hz_w; a.hz_b = ma.hz_b; a.inv_obs = ma.inv_obs;
    a.lik_scale = ma.lik_scale; a.obs_scale = ma.obs_scale; a.nh_inv_var = ma.nh_inv_var; a.ll_const = ma.ll_const;
    const int nc = (a.half + 63) / 64;   // <= 17 at D = 2049
    unsigned blocks = cdiv(rows, D3P_GN_WAVES);
    blocks = blocks > D3P_GN_MAX_BLOCKS ? D3P_GN_MAX_BLOCKS : blocks;
    const size_t lds = (size_t)5 * D * sizeof(float);
    if (model->family == D3P_FAMILY_LINREG) gn_launch<D3P_FAMILY_LINREG>(s, nc, dim3(blocks), lds, a);
    else if (model->family == D3P_FAMILY_POISSON) gn_launch<D3P_FAMILY_POISSON>(s, nc, dim3(blocks), lds, a);
    else gn_launch<D3P_FAMILY_LOGREG>(s, nc, dim3(blocks), lds, a);
    return check_launch(what);
}

size_t d3p_norm_profile_workspace(uint64_t n)
{
    return NP_HIST_BYTES + NP_STATE_BYTES + (size_t)np_strips(n) * D3P_NP_PART_WORDS * 8;
}

int d3p_norm_profile(void* stream, const float* norms_dev, uint64_t n, uint32_t m, const float* thresholds_host, uint32_t Q,
                     const uint64_t* lo_host, const double* g_host, void* out_dev, void* workspace_dev, size_t workspace_bytes)
{
    const char* what = "d3p_norm_profile";
    if (!norms_dev || !out_dev || !workspace_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n >= 1 is required", what);
    if (n > D3P_NP_MAX_N) return fail(D3P_E_UNSUPPORTED, "%s: n <= 2^40 (n = %llu)", what, (unsigned long long)n);
    if (m > D3P_NP_MAX) return fail(D3P_E_INVALID_ARG, "%s: at most 8 thresholds (m = %u)", what, m);
    if (Q > D3P_NP_MAX) return fail(D3P_E_INVALID_ARG, "%s: at most 8 quantile positions (Q = %u)", what, Q);
    if ((m && !thresholds_host) || (Q && (!lo_host || !g_host))) return fail(D3P_E_INVALID_ARG, "%s: null host array", what);
    if ((m && is_device_ptr(thresholds_host)) || (Q && (is_device_ptr(lo_host) || is_device_ptr(g_host))))
        return fail(D3P_E_INVALID_ARG, "%s: thresholds_host, lo_host and g_host must be host memory", what);
    if (((uintptr_t)norms_dev & 3u) || ((uintptr_t)out_dev & 7u) || ((uintptr_t)workspace_dev & 7u))
        return fail(D3P_E_INVALID_ARG, "%s: norms_dev must be aligned to 4 bytes, out_dev and workspace_dev to 8", what);
    NormProfArgs a;
    memset(&a, 0, sizeof(a));
    for (uint32_t k = 0; k < m; ++k) {
        const float c = thresholds_host[k];
        if (!(c > 0.f && std::isfinite(c))) return fail(D3P_E_INVALID_ARG, "%s: threshold[%u] = %g must be finite and > 0", what, k, (double)c);
        a.thr[k] = c;
    }
    for (uint32_t q = 0; q < Q; ++q) {
        const uint64_t lo = lo_host[q];
        const double g = g_host[q];
        if (lo >= n) return fail(D3P_E_INVALID_ARG, "%s: lo[%u] = %llu is not below n = %llu", what, q, (unsigned long long)lo, (unsigned long long)n);
        if (!(g >= 0.0 && g < 1.0)) return fail(D3P_E_INVALID_ARG, "%s: g[%u] = %g is outside [0, 1)", what, q, g);
        a.lo[q] = lo;
        a.g[q] = g;
    }
    if (workspace_bytes < d3p_norm_profile_workspace(n))
        return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace_bytes, d3p_norm_profile_workspace(n));
    if (!is_device_ptr(norms_dev) || !is_device_ptr(out_dev) || !is_device_ptr(workspace_dev))
        return fail(D3P_E_INVALID_ARG, "%s: norms_dev, out_dev and workspace_dev must be device memory", what);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t strips = np_strips(n);
    a.v = reinterpret_cast<const uint32_t*>(norms_dev);
    a.n = n;
    a.strip_len = (n + strips - 1) / strips;
    a.m = m; a.Q = Q; a.R = 2 * Q;
    a.hist = static_cast<unsigned long long*>(workspace_dev);
    a.state = reinterpret_cast<NpState*>(static_cast<char*>(workspace_dev) + NP_HIST_BYTES);
    a.parts = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace_dev) + NP_HIST_BYTES + NP_STATE_BYTES);
    a.out = static_cast<unsigned long long*>(out_dev);
    D3P_HIP_TRY(hipMemsetAsync(workspace_dev, 0, NP_HIST_BYTES, s));
    hipLaunchKernelGGL(k_norm_pass<0>, dim3(strips), dim3(256), 0, s, a);
    if (Q) {
        hipLaunchKernelGGL(k_norm_pass<1>, dim3(strips), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_norm_pass<2>, dim3(strips), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_norm_pass<3>, dim3(strips), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(k_norm_final, dim3(1), dim3(256), 0, s, a, strips);
    return check_launch(what);
}

}  // extern "C"
