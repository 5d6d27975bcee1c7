// Credible and predictive intervals (d3p_amd/intervals.py, include/d3p_hip.h): per-column quantiles of a draws x cols
// matrix, d3p_col_quantiles, and the rows form of the regression families' conditional mean, d3p_predict_mean_rows, which writes the
// matrix the first reduces for a credible interval.
//
// k_col_quantiles knows nothing of the model.  The host hands it, per requested probability, a position (lo, g): the result lies
// between the (lo+1)-th and the (lo+2)-th smallest value of the column, a fraction g of the way (numpy's method='linear').  Both order
// statistics are found EXACTLY on the stored values through an order-preserving uint32 key (key_of, d3p_colreduce.h: float32 with -0
// taken as +0; int32: u ^ 0x80000000), so the only arithmetic is the interpolation, in float64, rounded to float32 once.
//
// One workgroup of 256 threads owns D3P_Q_COLS = 32 adjacent columns (one 128-byte line of every draw's row of the matrix), k_psis_loo's
// geometry: thread t = (draw lane t / 32, column lane t % 32), the 8 draw lanes of a column take the draws dl, dl + 8, ...
//   pass 0       every value once: the NaN flag of the column and, in the staged form, its key into LDS ([draw][32 columns]: the 32
//                lanes of a half-wave write and read 32 consecutive words, no bank conflict).
//   per (lo, g)  four 8-bit radix passes, most significant byte first, over a 32 x 257 uint32 histogram (integer LDS atomics; 257 puts
//                the 32 column lanes of an update on 32 banks): the key of a.  The bin of the wanted rank is found by the column's 8
//                draw lanes together: each sums 32 bins, the lane whose range holds the rank walks its 32 bins again.  Where g != 0 ONE
//                more pass counts the keys <= key(a) and takes the smallest key above it: b = a if the count reaches lo + 2, else that
//                minimum.  Five passes per probability instead of eight.
// Staged form (n <= D3P_Q_STAGED_MAX = 895: histogram + 32 n keys <= 144 KiB of dynamic LDS): every pass after pass 0 reads LDS.
// Streamed form (n above that): every pass reads the column from memory again, a wave two whole lines per load.
// Both forms select the same keys -- the selection is exact -- so a column's output bits depend on its values and (n, lo, g) alone:
// not on ld, out_ld, the other columns of the launch or the form.  No floating-point atomics; a column past the end stands for n
// draws of 0 and writes nothing.
//
// k_mean_rows is the sixth user of the draws x rows product tile (d3p_glm_tile.h) with k_loglik's rows-form grid (row tiles x draw
// tiles) and store (64 consecutive floats per wave), and the link k_moments has: mu = glm_mean<FAMILY>(t) (d3p_glm_tile.h).
#include "d3p_colreduce.h"
#include "d3p_device.h"
#include "d3p_glm_tile.h"

#pragma clang fp contract(off)

namespace d3p {

#define D3P_Q_COLS 32
#define D3P_Q_DL 8
#define D3P_Q_HSTRIDE 257             // 256 bins + 1: the 32 column lanes of a histogram update fall on 32 banks
#define D3P_Q_MAX 8                   // probabilities per launch
#define D3P_Q_HIST_BYTES (D3P_Q_COLS * D3P_Q_HSTRIDE * 4)
#define D3P_Q_STAGED_MAX ((D3P_DYN_LDS_MAX - D3P_Q_HIST_BYTES) / (D3P_Q_COLS * 4))   // 895 draws

struct QuantArgs {
    const uint32_t* m;   // the matrix's words: float32 or int32
    int32_t dtype;       // 0: float32, 1: int32
    int64_t ld;
    uint32_t n;
    uint64_t cols;
    uint32_t Q;
    uint32_t lo[D3P_Q_MAX];
    double g[D3P_Q_MAX];
    float* out;
    int64_t out_ld;
};

// the stored value of a key in float64: exact for both types
__device__ inline double q_value(uint32_t k, int32_t dtype) { return dtype ? (double)i32_of_key(k) : (double)f32_of_key(k); }

template <bool STAGED>
__global__ __launch_bounds__(256) void k_col_quantiles(QuantArgs a)
{
    extern __shared__ __align__(16) unsigned char q_smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(q_smem);                       // [32][257]
    uint32_t* keys = reinterpret_cast<uint32_t*>(q_smem + D3P_Q_HIST_BYTES);    // staged form: [n][32]

    __shared__ uint32_t r_u0[D3P_Q_DL][D3P_Q_COLS], r_u1[D3P_Q_DL][D3P_Q_COLS];
    __shared__ uint32_t s_prefix[D3P_Q_COLS], s_rank[D3P_Q_COLS];

    const int t = threadIdx.x, cl = t & (D3P_Q_COLS - 1), dl = t >> 5;
    const uint32_t n = a.n;
    const int32_t dtype = a.dtype;
    const uint64_t c = (uint64_t)blockIdx.x * D3P_Q_COLS + cl;
    const bool live = c < a.cols;                       // a column past the end stands for n draws of 0 and writes nothing
    const uint32_t* col = a.m + (live ? c : 0);
    const size_t ld = (size_t)a.ld;
#define Q_LOAD(s) (live ? col[(size_t)(s) * ld] : 0u)
#define Q_KEY(s) (STAGED ? keys[(size_t)(s) * D3P_Q_COLS + cl] : key_of(Q_LOAD(s), dtype))

    // pass 0: the column's NaN flag; the staged form keeps the keys
    uint32_t nan = 0u;
    for (uint32_t s = dl; s < n; s += D3P_Q_DL) {
        const uint32_t u = Q_LOAD(s);
        if (!dtype && word_is_nan(u)) nan = 1u;
        if (STAGED) keys[(size_t)s * D3P_Q_COLS + cl] = key_of(u, dtype);
    }
    r_u0[dl][cl] = nan;
    __syncthreads();
    for (int q = 0; q < D3P_Q_DL; ++q) nan |= r_u0[q][cl];
    __syncthreads();

    for (uint32_t qi = 0; qi < a.Q; ++qi) {
        const uint32_t lo = a.lo[qi];
        const double g = a.g[qi];
        // the radix select of the (lo+1)-th smallest key
        for (int p = 0; p < 4; ++p) {
            for (int i = t; i < D3P_Q_COLS * D3P_Q_HSTRIDE; i += 256) hist[i] = 0u;
            __syncthreads();
            const int shift = 24 - 8 * p;
            const uint32_t prefix = p ? s_prefix[cl] : 0u;
            const uint32_t want = p ? s_rank[cl] : lo + 1u;
            for (uint32_t s = dl; s < n; s += D3P_Q_DL) {
                const uint32_t key = Q_KEY(s);
                if (p == 0) atomicAdd(&hist[cl * D3P_Q_HSTRIDE + (key >> 24)], 1u);
                else if ((key >> (shift + 8)) == prefix) atomicAdd(&hist[cl * D3P_Q_HSTRIDE + ((key >> shift) & 255u)], 1u);
            }
            __syncthreads();
            // draw lane dl owns the bins 32 dl .. 32 dl + 31 of its column
            const uint32_t* h = hist + cl * D3P_Q_HSTRIDE + dl * 32;
            uint32_t mine = 0u;
#pragma unroll
            for (int j = 0; j < 32; ++j) mine += h[j];
            r_u0[dl][cl] = mine;
            __syncthreads();
            uint32_t before = 0u;
            for (int q = 0; q < D3P_Q_DL; ++q) before += q < dl ? r_u0[q][cl] : 0u;
            if (before < want && want <= before + mine) {   // exactly one lane of the column: the bins hold >= want keys in all
                uint32_t cum = before, bin = 0u, rank = 1u;
                bool found = false;
#pragma unroll
                for (int j = 0; j < 32; ++j) {
                    const uint32_t cnt = h[j];
                    if (!found && cum + cnt >= want) { found = true; bin = (uint32_t)j; rank = want - cum; }
                    cum += cnt;
                }
                s_prefix[cl] = (prefix << 8) | ((uint32_t)dl * 32u + bin);
                s_rank[cl] = rank;
            }
            __syncthreads();
        }
        const uint32_t ka = s_prefix[cl];
        uint32_t kb = ka;
        if (g != 0.0) {   // (uniform: g is a kernel argument)
            uint32_t cnt = 0u, above = 0xffffffffu;
            for (uint32_t s = dl; s < n; s += D3P_Q_DL) {
                const uint32_t key = Q_KEY(s);
                if (key <= ka) ++cnt;
                else above = key < above ? key : above;
            }
            r_u0[dl][cl] = cnt; r_u1[dl][cl] = above;
            __syncthreads();
            cnt = 0u; above = 0xffffffffu;
            for (int q = 0; q < D3P_Q_DL; ++q) { cnt += r_u0[q][cl]; above = r_u1[q][cl] < above ? r_u1[q][cl] : above; }
            if (cnt < lo + 2u) kb = above;   // (lo + 2 <= n where g != 0: a key above exists)
        }
        if (dl == 0 && live) {
            const double va = q_value(ka, dtype), vb = q_value(kb, dtype);
            const double res = lerp_linear(va, vb, g);
            a.out[(size_t)qi * (size_t)a.out_ld + c] = nan ? NAN : (float)res;
        }
        __syncthreads();   // (r_u0 / r_u1, s_prefix and s_rank are free for the next probability)
    }
#undef Q_KEY
#undef Q_LOAD
}

// ---- the conditional mean over posterior draws, rows form -------------------------------------------------------------------------
struct MeanRowsArgs {
    const float* X;
    uint64_t rows;
    int d, w_off, b_col;
    const float* lat;
    int64_t ld;
    uint32_t n;
    float* out;
    int64_t out_ld;
};

template <int FAMILY>
// Registers: two waves per SIMD as k_loglik's rows form (one draw tile per workgroup: nothing lives across a loop); no scratch.
__global__ void __launch_bounds__(256, 2) k_mean_rows(MeanRowsArgs g)
{
    // [k][draw] | [k][row] during the product; afterwards the same bytes hold each wave's t, half a tile at a time (4 x 32 x 65 floats)
    __shared__ __attribute__((aligned(16))) float smem[D3P_TILE_SMEM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const uint64_t r0 = (uint64_t)blockIdx.x * D3P_TILE_N;
    const uint32_t s0 = blockIdx.y * D3P_TILE_M;
    const uint64_t r = r0 + wn * 64 + lane;   // lane l owns row r in the epilogue
    const bool live = r < g.rows;
    tile_f16v acc[2][2];
    tile_product(smem, g, r0, s0, acc);
    float* L = tile_block(smem);
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
        tile_scatter(L, acc[mb][0], acc[mb][1]);
        __syncthreads();
        if (live) {
            for (int i = 0; i < 32; ++i) {
                const uint32_t s = s0 + wm * 64 + mb * 32 + i;
                if (s >= g.n) break;
                float t = L[i * 65 + lane];
                if (g.b_col >= 0) t = t + g.lat[(size_t)s * g.ld + g.b_col];
                g.out[(size_t)s * (size_t)g.out_ld + r] = glm_mean<FAMILY>(t);
            }
        }
        __syncthreads();
    }
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_col_quantiles_staged_max(void) { return (uint32_t)D3P_Q_STAGED_MAX; }

int d3p_col_quantiles(void* stream, const void* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t cols, uint32_t Q, const uint32_t* lo_host,
                      const double* g_host, float* out_dev, int64_t out_ld)
{
    const char* what = "d3p_col_quantiles";
    if (!m_dev || !out_dev || !lo_host || !g_host) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if (!aligned4(m_dev) || !aligned4(out_dev)) return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (n < 1 || n > 65535u) return fail(D3P_E_INVALID_ARG, "%s: 1 <= n <= 65535 (n = %u)", what, n);
    if (Q < 1 || Q > D3P_Q_MAX) return fail(D3P_E_INVALID_ARG, "%s: 1 <= Q <= 8 (Q = %u)", what, Q);
    if (is_device_ptr(lo_host) || is_device_ptr(g_host)) return fail(D3P_E_INVALID_ARG, "%s: lo_host and g_host must be host memory", what);
    QuantArgs a;
    for (uint32_t q = 0; q < Q; ++q) {
        const uint32_t lo = lo_host[q];
        const double g = g_host[q];
        if (lo >= n) return fail(D3P_E_INVALID_ARG, "%s: lo[%u] = %u is not below n = %u", what, q, lo, n);
        if (!(g >= 0.0 && g < 1.0)) return fail(D3P_E_INVALID_ARG, "%s: g[%u] = %g is outside [0, 1)", what, q, g);
        if (g != 0.0 && lo == n - 1) return fail(D3P_E_INVALID_ARG, "%s: g[%u] must be 0 at lo = n - 1 (there is no value above the largest)", what, q);
        a.lo[q] = lo;
        a.g[q] = g;
    }
    for (uint32_t q = Q; q < D3P_Q_MAX; ++q) { a.lo[q] = 0u; a.g[q] = 0.0; }
    if (ld < 0 || (uint64_t)ld < cols) return fail(D3P_E_INVALID_ARG, "%s: ld >= cols is required", what);
    if (out_ld < 0 || (uint64_t)out_ld < cols) return fail(D3P_E_INVALID_ARG, "%s: out_ld >= cols is required", what);
    if (cols == 0) return D3P_OK;
    if (cols > (uint64_t)0x7fffffff * D3P_Q_COLS) return fail(D3P_E_UNSUPPORTED, "%s: cols <= 32 (2^31 - 1)", what);
    if (!is_device_ptr(m_dev) || !is_device_ptr(out_dev)) return fail(D3P_E_INVALID_ARG, "%s: the matrix and the output must be device memory", what);
    a.m = static_cast<const uint32_t*>(m_dev); a.dtype = dtype; a.ld = ld; a.n = n; a.cols = cols; a.Q = Q; a.out = out_dev; a.out_ld = out_ld;
    const dim3 grid((unsigned)((cols + D3P_Q_COLS - 1) / D3P_Q_COLS));
    if (n <= D3P_Q_STAGED_MAX) {
        const size_t lds = (size_t)D3P_Q_HIST_BYTES + (size_t)D3P_Q_COLS * n * 4;
        if (lds > 48u * 1024u)
            if (int rc = dynamic_lds_opt_in(reinterpret_cast<const void*>(&k_col_quantiles<true>), D3P_DYN_LDS_MAX, what)) return rc;
        hipLaunchKernelGGL((k_col_quantiles<true>), grid, dim3(256), lds, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL((k_col_quantiles<false>), grid, dim3(256), (size_t)D3P_Q_HIST_BYTES, (hipStream_t)stream, a);
    }
    return check_launch(what);
}

int d3p_predict_mean_rows(void* stream, const d3p_logreg_model* model, const float* X_dev, uint64_t rows, const float* latent_dev,
                          int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, float* out_dev, int64_t out_ld)
{
    const char* what = "d3p_predict_mean_rows";
    const d3p_logreg_model* m = model;
    // (there are no labels: validate_model's label check gets a pointer that is not null)
    if (int rc = validate_model(m, m, what)) return rc;   // D3P_GUIDE_EXP_SITES: D3P_E_UNSUPPORTED (the guide transform is not read otherwise)
    bool launch;
    if (int rc = glm_tile_check(what, m, rows, latent_ld, w_off, b_col, n, {X_dev, latent_dev, out_dev}, "X / latent / out", "X, latent and out", &launch))
        return rc;
    if (out_ld < 0 || (uint64_t)out_ld < rows) return fail(D3P_E_INVALID_ARG, "%s: out_ld >= rows is required", what);
    if (!launch) return D3P_OK;
    MeanRowsArgs g;
    g.X = X_dev; g.rows = rows; g.d = m->d; g.w_off = w_off; g.b_col = b_col; g.lat = latent_dev; g.ld = latent_ld; g.n = n;
    g.out = out_dev; g.out_ld = out_ld;
    const dim3 grid(cdiv(rows, D3P_TILE_N), cdiv(n, D3P_TILE_M));
    hipStream_t s = (hipStream_t)stream;
    if (m->family == D3P_FAMILY_LINREG) hipLaunchKernelGGL((k_mean_rows<D3P_FAMILY_LINREG>), grid, dim3(256), 0, s, g);
    else if (m->family == D3P_FAMILY_POISSON) hipLaunchKernelGGL((k_mean_rows<D3P_FAMILY_POISSON>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((k_mean_rows<D3P_FAMILY_LOGREG>), grid, dim3(256), 0, s, g);
    return check_launch(what);
}

}  // extern "C"
