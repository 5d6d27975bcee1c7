// Importance-weighted held-out log-likelihood of the VAE (d3p_amd/vae_density.py): the log importance weights
//   log_w[i, b] = log p(x_b | z_ib) + log p(z_ib) - log q(z_ib | x_b),   z_ib ~ q(. | x_b) = Normal(zl_b, exp(zs_b))
// of n guide draws per image (Burda, Grosse & Salakhutdinov 2016), and the per-column statistics of a draws x columns matrix that
// turn them into the per-image ELBO, the importance-weighted bound and the effective sample size.  All quantities are UNSCALED.
//
// d3p_vae_log_weights is unfused on purpose: the encoder runs once, d3p_predict_draws draws z under the posterior predictive's key
// rule, and the decoder (the product kernels of d3p_gemm.hip through vae_predict_decode) writes the logits of one SLAB of draws at a
// time; k_vae_logw reads a slab's logits back and reduces each row.  (The logits round trip is 4 D bytes per row beside about
// 2 (Z H + H D) flops of products: docs/experiments_vae_density.md has the measured share.)
//
// k_vae_logw: one wavefront per row (row = i B + b), four rows per workgroup, no LDS, no barrier, no atomics.  Lane l owns the
// elements c with (c / 4) mod 64 == l (groups of four consecutive columns), walks them in ascending order and adds each term to a
// float64 lane sum; the 64 lane sums are merged by the xor butterfly 32, 16, 8, 4, 2, 1 (every lane ends with the same bits).  The
// element-to-lane map is the same whether the four columns arrive as one 16-byte load (D % 4 == 0 and both row starts aligned) or as
// scalar loads, so the output bits do not depend on the load path: they are a function of the arguments' values alone.  The Z terms
// are walked at lane stride 64.  Per-term arithmetic is float32 with every operation rounded on its own (fp contract off):
//   px term  x a - (max(a, 0) + log(1 + exp(-|a|)))          the softplus of the output product's epilogue 4 (d3p_gemm.hip), __expf / __logf
//   pz term  (-0.5 (z z)) - HALF_LOG_2PI
//   qz term  ((-0.5 (u u)) - zs) - HALF_LOG_2PI,  u = (z - zl) expf(-zs)
// log_w = (px + pz) - qz in float64, rounded to float32 once; the parts are the float64 sums rounded to float32 once each.
// Rows past `rows` are handled by clamping the row that is read and masking the stores (selects, not an early return).
//
// k_col_stats: model-free.  64 columns per workgroup (lane = column: a wavefront reads 256 consecutive bytes of a draw), the draws cut
// into four contiguous chunks of ceil(n / 4), one per wavefront, each walked in ascending draw order in float64; the four chunk
// results are merged by thread w = 0 of each column in the order ((c0 + c1) + c2) + c3.  Two sweeps over the column: sum and max, then
// the centred squares and r = exp(v - max).
#include "d3p_device.h"
#include "d3p_host.h"

#pragma clang fp contract(off)

namespace d3p {

int vae_predict_encode(hipStream_t s, const d3p_vae_model* m, const float* params, const float* X, uint32_t B, float* zl, float* zs, float* h0, float* h1,
                       float* sg);
int vae_predict_decode(hipStream_t s, const d3p_vae_model* m, const float* params, const float* z, uint32_t rows, float* logits, float* h0, float* h1,
                       float* sg);

#define D3P_LOGW_WAVES 4
#define D3P_HALF_LOG_2PI_F 0.918938533204672742f

struct LogwArgs {
    const float* logits;   // rows x D: the slab's output pre-activations
    const float* X;        // B x D
    const float* z;        // rows x Z: the slab's latents
    const float *zl, *zs;  // B x Z: the guide's loc and log scale
    uint32_t rows, B;      // a slab starts at a whole draw: image b = row mod B
    int D, Z, vec;
    float *logw, *px, *pz, *qz;   // the slab's outputs (rows each; the parts optional)
};

__device__ __forceinline__ double logw_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Bernoulli(logits = a).log_prob(x) = x a - softplus(a), as epilogue 4 of the output product evaluates its terms
__device__ __forceinline__ float logw_px_term(float x, float a)
{
    const float en = __expf(-fabsf(a));
    const float sp = fmaxf(a, 0.0f) + __logf(1.0f + en);
    const float xa = x * a;
    return xa - sp;
}

__global__ void __launch_bounds__(64 * D3P_LOGW_WAVES) k_vae_logw(LogwArgs g)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t row_raw = blockIdx.x * D3P_LOGW_WAVES + wave;
    const bool live = row_raw < g.rows;
    const uint32_t row = live ? row_raw : g.rows - 1;   // a dead wavefront recomputes the last row and stores nothing
    const uint32_t b = row % g.B;
    const float* lr = g.logits + (size_t)row * g.D;
    const float* xr = g.X + (size_t)b * g.D;
    double spx = 0.0;
    const int D4 = g.D & ~3;
    if (g.vec) {
        for (int c = 4 * lane; c < D4; c += 256) {
            const float4 a = *reinterpret_cast<const float4*>(lr + c);
            const float4 x = *reinterpret_cast<const float4*>(xr + c);
            spx += (double)logw_px_term(x.x, a.x);
            spx += (double)logw_px_term(x.y, a.y);
            spx += (double)logw_px_term(x.z, a.z);
            spx += (double)logw_px_term(x.w, a.w);
        }
    } else {
        for (int c = 4 * lane; c < D4; c += 256) {
#pragma unroll
            for (int k = 0; k < 4; ++k) spx += (double)logw_px_term(xr[c + k], lr[c + k]);
        }
    }
    {   // the last group of a row whose length is no multiple of four: its owner lane, after its whole groups
        const int c = D4;
        if (c < g.D && ((c >> 2) & 63) == lane)
            for (int k = 0; c + k < g.D; ++k) spx += (double)logw_px_term(xr[c + k], lr[c + k]);
    }
    double spz = 0.0, sqz = 0.0;
    const float* zr = g.z + (size_t)row * g.Z;
    const float* zlr = g.zl + (size_t)b * g.Z;
    const float* zsr = g.zs + (size_t)b * g.Z;
    for (int j = lane; j < g.Z; j += 64) {
        const float z = zr[j], zl = zlr[j], zs = zsr[j];
        const float zz = z * z;
        const float tp = -0.5f * zz - D3P_HALF_LOG_2PI_F;
        const float dz = z - zl;
        const float u = dz * expf(-zs);
        const float uu = u * u;
        const float tq = (-0.5f * uu - zs) - D3P_HALF_LOG_2PI_F;
        spz += (double)tp;
        sqz += (double)tq;
    }
    spx = logw_wave_sum(spx);
    spz = logw_wave_sum(spz);
    sqz = logw_wave_sum(sqz);
    if (live && lane == 0) {
        g.logw[row] = (float)((spx + spz) - sqz);
        if (g.px) {
            g.px[row] = (float)spx;
            g.pz[row] = (float)spz;
            g.qz[row] = (float)sqz;
        }
    }
}

// ---- column statistics ----------------------------------------------------------------------------------------------------------
struct ColStatsArgs {
    const float* m;
    int64_t ld;
    uint32_t n, cols, chunk;   // chunk = ceil(n / 4) draws per wavefront
    double* out;               // [4][cols]: mean, var (ddof 1), logsumexp - log n, ess
};

__global__ void __launch_bounds__(256) k_col_stats(ColStatsArgs g)
{
    __shared__ double red[3][4][64];
    __shared__ int nan_flag[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t col_raw = blockIdx.x * 64u + lane;
    const bool live = col_raw < g.cols;
    const uint32_t col = live ? col_raw : g.cols - 1;
    const uint32_t lo = wave * g.chunk < g.n ? wave * g.chunk : g.n;
    const uint32_t hi = lo + g.chunk < g.n ? lo + g.chunk : g.n;
    const float* p = g.m + col;
    // sweep 1: sum, max and whether a NaN was seen
    double s = 0.0, mx = -INFINITY;
    int nan = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        const double v = (double)p[(size_t)i * g.ld];
        nan |= v != v;
        s += v;
        mx = fmax(mx, v);
    }
    red[0][wave][lane] = s;
    red[1][wave][lane] = mx;
    nan_flag[wave][lane] = nan;
    __syncthreads();
    const double dn = (double)g.n;
    const double S = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
    const double MX = fmax(fmax(red[1][0][lane], red[1][1][lane]), fmax(red[1][2][lane], red[1][3][lane]));
    const int any_nan = nan_flag[0][lane] | nan_flag[1][lane] | nan_flag[2][lane] | nan_flag[3][lane];
    const double mean = S / dn;
    __syncthreads();
    // sweep 2: centred squares, sum r and sum r^2 with r = exp(v - max); a column whose max is not finite has no r
    const bool mx_finite = MX - MX == 0.0;
    double q = 0.0, r1 = 0.0, r2 = 0.0;
    for (uint32_t i = lo; i < hi; ++i) {
        const double v = (double)p[(size_t)i * g.ld];
        const double dv = v - mean;
        q += dv * dv;
        const double r = exp(mx_finite ? v - MX : 0.0);
        r1 += r;
        r2 += r * r;
    }
    red[0][wave][lane] = q;
    red[1][wave][lane] = r1;
    red[2][wave][lane] = r2;
    __syncthreads();
    if (wave == 0 && live) {
        const double Q = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
        const double R1 = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
        const double R2 = ((red[2][0][lane] + red[2][1][lane]) + red[2][2][lane]) + red[2][3][lane];
        const double nan_v = __longlong_as_double(0x7ff8000000000000ll);
        double var = Q / (dn - 1.0);   // one draw: 0 / 0 = NaN
        double lse = mx_finite ? MX + log(R1) - log(dn) : MX;   // every draw -inf: -inf; a +inf draw: +inf
        double ess = mx_finite ? (R1 * R1) / R2 : nan_v;
        double mean_o = mean;
        if (any_nan) mean_o = var = lse = ess = nan_v;
        g.out[col] = mean_o;
        g.out[(size_t)g.cols + col] = var;
        g.out[2 * (size_t)g.cols + col] = lse;
        g.out[3 * (size_t)g.cols + col] = ess;
    }
}

// ---- the slabs of d3p_vae_log_weights -------------------------------------------------------------------------------------------
// The product dispatcher of d3p_gemm.hip picks its kernel by the row count of a product (more than 96 rows: the bf16x3 kernel), and the
// two kernels round differently.  For outputs that do not depend on draws_per_slab every slab must therefore fall on the side of that
// threshold on which the whole call's n B rows fall: n B <= D3P_LOGW_SMALL_ROWS runs as ONE slab; otherwise a slab holds at least
// `floor_draws` = ceil((D3P_LOGW_SMALL_ROWS + 1) / B) draws, and a remainder shorter than that joins the slab before it.
#define D3P_LOGW_SMALL_ROWS 96u

struct LogwSlabs { uint32_t per, floor_draws, max_draws; };

static LogwSlabs logw_slabs(uint32_t B, uint32_t draws_per_slab)
{
    LogwSlabs s;
    s.floor_draws = (D3P_LOGW_SMALL_ROWS + 1 + B - 1) / B;
    s.per = draws_per_slab > s.floor_draws ? draws_per_slab : s.floor_draws;
    s.max_draws = s.per + s.floor_draws - 1;   // a slab plus a joined remainder; also >= any n with n B <= D3P_LOGW_SMALL_ROWS
    return s;
}

struct LogwWs { float *zl, *zs, *h0, *h1, *sg, *logits; };

static size_t logw_carve(const d3p_vae_model* m, uint32_t B, uint32_t slab_draws, char* base, LogwWs* w)
{
    const size_t R = (size_t)B * slab_draws, hmax = (size_t)(m->H > m->H2 ? m->H : m->H2);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) / 256 * 256; return p; };
    LogwWs t;
    t.zl = (float*)take((size_t)B * m->Z * 4);
    t.zs = (float*)take((size_t)B * m->Z * 4);
    t.h0 = (float*)take(R * hmax * 4);
    t.h1 = (float*)take(R * hmax * 4);
    t.sg = (float*)take(R * hmax * 4);
    t.logits = (float*)take(R * (size_t)m->D * 4);
    if (w) *w = t;
    return off;
}

static inline bool logw_model_ok(const d3p_vae_model* m) { return m && m->D >= 1 && m->H >= 1 && m->Z >= 1 && m->H2 >= 0; }

}  // namespace d3p

using namespace d3p;

extern "C" {

size_t d3p_vae_log_weights_workspace(const d3p_vae_model* model, uint32_t B, uint32_t draws_per_slab)
{
    if (!logw_model_ok(model) || B < 1 || draws_per_slab < 1) return 0;
    const LogwSlabs sl = logw_slabs(B, draws_per_slab);
    if ((uint64_t)sl.max_draws * B > 0x7fffffffull) return 0;
    return logw_carve(model, B, sl.max_draws, nullptr, nullptr);
}

int d3p_vae_log_weights(void* stream, const d3p_vae_model* model, const float* params_dev, const float* X_dev, uint32_t B, const uint32_t* key_dev,
                        uint32_t n, int32_t multi, uint32_t draws_per_slab, float* z_out_dev, float* logw_out_dev, float* parts_out_dev,
                        void* workspace_dev, size_t workspace_bytes)
{
    D3P_REQUIRE(logw_model_ok(model), "d3p_vae_log_weights: bad model");
    D3P_REQUIRE(B >= 1 && n >= 1 && (uint64_t)B * n <= 0x7fffffffull, "d3p_vae_log_weights: 1 <= B, n and n B < 2^31");
    D3P_REQUIRE((uint64_t)B * model->D <= 0xFFFFFFFFull && (uint64_t)B * model->Z <= 0x7fffffffull, "d3p_vae_log_weights: B too large");
    D3P_REQUIRE((uint64_t)B * n * model->Z <= (1ull << 40), "d3p_vae_log_weights: n B Z too large");
    D3P_REQUIRE(draws_per_slab >= 1, "d3p_vae_log_weights: draws_per_slab >= 1");
    const LogwSlabs sl = logw_slabs(B, draws_per_slab);
    const uint32_t ws_draws = sl.max_draws < n ? sl.max_draws : n;   // (the workspace entry does not know n: it sizes for max_draws)
    D3P_REQUIRE((uint64_t)ws_draws * B * model->D <= (1ull << 38), "d3p_vae_log_weights: a slab of draws_per_slab B D values is too large");
    D3P_REQUIRE_DEV(key_dev, "d3p_vae_log_weights: key_dev must be device memory");
    D3P_REQUIRE_DEV(params_dev, "d3p_vae_log_weights: params_dev must be device memory");
    D3P_REQUIRE_DEV(X_dev, "d3p_vae_log_weights: X_dev must be device memory");
    D3P_REQUIRE_DEV(z_out_dev, "d3p_vae_log_weights: z_out_dev must be device memory");
    D3P_REQUIRE_DEV(logw_out_dev, "d3p_vae_log_weights: logw_out_dev must be device memory");
    if (parts_out_dev) D3P_REQUIRE_DEV(parts_out_dev, "d3p_vae_log_weights: parts_out_dev must be device memory");
    D3P_REQUIRE_DEV(workspace_dev, "d3p_vae_log_weights: workspace_dev must be device memory");
    const size_t need = d3p_vae_log_weights_workspace(model, B, draws_per_slab);
    if (need == 0 || workspace_bytes < need) return fail(D3P_E_WORKSPACE, "d3p_vae_log_weights: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    LogwWs w;
    logw_carve(model, B, sl.max_draws, (char*)workspace_dev, &w);
    // the site plan of d3p_predict_vae's posterior branch: the guide's z (guide chain, key 0), Normal(zl, exp(zs)); the obs site's key is not needed
    d3p_predict_site zsite;
    memset(&zsite, 0, sizeof(zsite));
    zsite.size = (int32_t)(B * (uint32_t)model->Z);
    zsite.offset = 0; zsite.chain = 1; zsite.key_index = 0;
    zsite.scale_kind = D3P_PREDICT_SCALE_EXP;
    zsite.loc_c = 0.f; zsite.scale_c = 1.f;
    zsite.loc_dev = w.zl; zsite.scale_dev = w.zs;
    if (int rc = vae_predict_encode(s, model, params_dev, X_dev, B, w.zl, w.zs, w.h0, w.h1, w.sg)) return rc;
    if (int rc = d3p_predict_draws(stream, key_dev, n, multi, 1, &zsite, 1, 0, 0, z_out_dev, zsite.size, nullptr)) return rc;
    const size_t total = (size_t)n * B;
    const bool al = (((uintptr_t)X_dev | (uintptr_t)w.logits) & 15u) == 0;
    uint32_t i0 = 0;
    while (i0 < n) {
        uint32_t cnt = n - i0 < sl.per ? n - i0 : sl.per;
        if (n - i0 - cnt < sl.floor_draws) cnt = n - i0;   // a short remainder joins this slab (and n B <= 96 is one slab)
        const uint32_t rows = cnt * B;
        const size_t r0 = (size_t)i0 * B;
        const float* zslab = z_out_dev + r0 * model->Z;
        if (int rc = vae_predict_decode(s, model, params_dev, zslab, rows, w.logits, w.h0, w.h1, w.sg)) return rc;
        LogwArgs g;
        g.logits = w.logits; g.X = X_dev; g.z = zslab; g.zl = w.zl; g.zs = w.zs;
        g.rows = rows; g.B = B; g.D = model->D; g.Z = model->Z;
        g.vec = (al && model->D % 4 == 0) ? 1 : 0;
        g.logw = logw_out_dev + r0;
        g.px = parts_out_dev ? parts_out_dev + r0 : nullptr;
        g.pz = parts_out_dev ? parts_out_dev + total + r0 : nullptr;
        g.qz = parts_out_dev ? parts_out_dev + 2 * total + r0 : nullptr;
        hipLaunchKernelGGL(k_vae_logw, dim3(cdiv(rows, D3P_LOGW_WAVES)), dim3(64 * D3P_LOGW_WAVES), 0, s, g);
        if (int rc = check_launch("d3p_vae_log_weights")) return rc;
        i0 += cnt;
    }
    return D3P_OK;
}

int d3p_vae_logw_rows(void* stream, const float* logits_dev, const float* X_dev, const float* z_dev, const float* zl_dev, const float* zs_dev,
                      uint32_t rows, uint32_t B, int32_t D, int32_t Z, float* logw_out_dev, float* parts_out_dev)
{
    const char* what = "d3p_vae_logw_rows";
    D3P_REQUIRE(rows >= 1 && rows <= 0x7fffffffu && B >= 1 && D >= 1 && Z >= 1, "d3p_vae_logw_rows: 1 <= rows < 2^31 and B, D, Z >= 1");
    D3P_REQUIRE((uint64_t)B * D <= 0xFFFFFFFFull && (uint64_t)B * Z <= 0x7fffffffull, "d3p_vae_logw_rows: B too large");
    for (const void* p : {(const void*)logits_dev, (const void*)X_dev, (const void*)z_dev, (const void*)zl_dev, (const void*)zs_dev, (const void*)logw_out_dev})
        if (!is_device_ptr(p)) return fail(D3P_E_INVALID_ARG, "%s: every pointer must be device memory", what);
    if (parts_out_dev) D3P_REQUIRE_DEV(parts_out_dev, "d3p_vae_logw_rows: parts_out_dev must be device memory");
    LogwArgs g;
    g.logits = logits_dev; g.X = X_dev; g.z = z_dev; g.zl = zl_dev; g.zs = zs_dev;
    g.rows = rows; g.B = B; g.D = D; g.Z = Z;
    g.vec = ((((uintptr_t)X_dev | (uintptr_t)logits_dev) & 15u) == 0 && D % 4 == 0) ? 1 : 0;
    g.logw = logw_out_dev;
    g.px = parts_out_dev;
    g.pz = parts_out_dev ? parts_out_dev + rows : nullptr;
    g.qz = parts_out_dev ? parts_out_dev + 2 * (size_t)rows : nullptr;
    hipLaunchKernelGGL(k_vae_logw, dim3(cdiv(rows, D3P_LOGW_WAVES)), dim3(64 * D3P_LOGW_WAVES), 0, (hipStream_t)stream, g);
    return check_launch(what);
}

int d3p_col_stats(void* stream, const float* m_dev, int64_t ld, uint32_t n, uint64_t cols, double* out_dev)
{
    const char* what = "d3p_col_stats";
    if (!m_dev || !out_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if (((uintptr_t)m_dev & 3u) || ((uintptr_t)out_dev & 7u)) return fail(D3P_E_INVALID_ARG, "%s: m must be aligned to 4 bytes, out to 8", what);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n >= 1", what);
    if (ld < 0 || (uint64_t)ld < cols) return fail(D3P_E_INVALID_ARG, "%s: ld >= cols is required", what);
    if (cols == 0) return D3P_OK;
    if (cols > 0x7fffffffull) return fail(D3P_E_UNSUPPORTED, "%s: cols < 2^31", what);
    if (!is_device_ptr(m_dev) || !is_device_ptr(out_dev)) return fail(D3P_E_INVALID_ARG, "%s: m and out must be device memory", what);
    ColStatsArgs g;
    g.m = m_dev; g.ld = ld; g.n = n; g.cols = (uint32_t)cols; g.chunk = (n + 3) / 4; g.out = out_dev;
    hipLaunchKernelGGL(k_col_stats, dim3(cdiv(cols, 64)), dim3(256), 0, (hipStream_t)stream, g);
    return check_launch(what);
}

}  // extern "C"
