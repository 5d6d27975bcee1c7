// Model weights for M candidate models from their pointwise elpd vectors (d3p_amd/model_weights.py, include/d3p_hip.h):
// stacking of predictive distributions by the EM fixed point (d3p_stacking_weights) and pseudo-BMA+ by the Bayesian bootstrap
// (d3p_bb_pseudo_bma).  Model-free: the input is a models x rows float32 matrix e[m * ld + r], 1 <= M <= 16; every value is widened to
// float64 on load and everything after that is float64.  The kernels are instantiated for MT = 4 and MT = 16 accumulators (M <= 4 runs
// the first): the per-model arrays are indexed by unrolled loops only, so they live in registers.
//
// Stacking.  Evaluation j at the current w (w = 1 / M at j = 0):
//   k_stack_strip<MT>   grid = strips, 256 lanes.  chunks = ceil(rows / 256); per = ceil(chunks / 512); strips = ceil(chunks / per)
//                       (<= 512): a function of rows alone.  Lane t of strip s takes the rows (s per + c) 256 + t, c = 0 .. per - 1, in
//                       ascending order; per row mx = max_m e, p_m = exp(e_m - mx) (float64 exp, recomputed in every evaluation: no
//                       rows x M array exists), den = sum_k w_k p_k by fused multiply-adds from 0.0 in ascending k, then
//                       acc_m += p_m / den and acc_f += mx + log(den).  The 256 lanes' M + 1 sums merge through LDS in one fixed
//                       tree (strides 128, 64, .. 1) and go to part[strip][0 .. M] (the last one f's).
//   k_stack_merge       one workgroup.  Thread v <= M adds part[.][v] in ascending strip order from strip 0's (the partials come
//                       through LDS, 256 strips at a time); g_m = sum / rows;
//                       gap = max_m g_m - 1; then the rule of the header: stop (done = 1, w_out and info_out written) where gap <= tol,
//                       where gap is NaN or where j == max_iter, else w_m <- w_m g_m and j + 1.
// Both read `done` first and return without writing when it is set: the host enqueues evaluations in chunks and reads the flag once per
// chunk, so launches enqueued behind the stopping one change nothing and the outputs do not depend on the chunk size.  No cooperative
// launch, no grid barrier, no kernel that waits on another workgroup.  A row with a NaN, a +inf, or -inf in every model gives a NaN p
// (e - mx is NaN there) and through den a NaN in every g: the gap is NaN and the run stops with every output NaN.
//
// Bayesian bootstrap.  g[b, r] = -log(1 - u[b, r]), u = bits_to_uniform(word (r & 1) of threefry2x32(key, (r >> 1, b)), 0, 1): a function
// of (key, b, r) alone.  u is a multiple of 2^-23 in [0, 1), so 1 - u is exact in float32 and lies in (0, 1]; THE LOGARITHM IS THE
// FLOAT64 log OF THAT VALUE (not logf, not a fast intrinsic): g carries the error of one float64 log and nothing else.
//   k_bb_sums<MT>       grid = (strips, ceil(B / 256)), lane = replicate, k_draw_sums' arrangement.  chunks = ceil(rows / 256);
//                       per = ceil(chunks / 128); strips = ceil(chunks / per) (<= 128, a function of rows alone).  A chunk's e values
//                       are staged once in LDS as float64 [m][row] and read as broadcasts; a lane walks the chunk's rows in ascending
//                       order, one threefry call per row pair, and keeps S += g and T_m = fma(g, e_m, T_m) (M + 1 float64
//                       accumulators); a term with g = 0 contributes 0 whatever e is (0 x -inf is not formed).  The thread that stages
//                       a row also checks it (NaN, +inf, or -inf in every model); a strip with such a row writes NaN for S.
//                       Partials: part[strip][v][b], v = 0 for S and 1 + m for T_m.
//   k_bb_replicate<MT>  one thread per replicate: the strips' partials in ascending strip order, z_m = (rows T_m) / S, z_out[b][m], and
//                       w_b = softmax(z) into wb[m][b].
//   k_bb_mean           one workgroup per model: lane t adds wb[m][t], wb[m][t + 256], .. in ascending order, the lanes merge in the
//                       fixed tree, w_out[m] = sum / B.
// The B x rows matrix is never written.  No atomics anywhere in this file.
#include "d3p_device.h"
#include "d3p_host.h"

namespace d3p {

#define D3P_MW_MAX_M 16
#define D3P_MW_LANES 256
#ifndef D3P_STACK_MAX_STRIPS
#define D3P_STACK_MAX_STRIPS 512   // (overridable for an A/B build; 128, 256 and 1024 were slower: docs/experiments_model_weights.md)
#endif
#define D3P_STACK_MERGE_TILE 256
#define D3P_BB_MAX_STRIPS 128
#define D3P_STACK_DEFAULT_CHUNK 128

// the workspace of a stacking run: the state, then part[strips][M + 1]
struct StackState {
    double w[D3P_MW_MAX_M];
    uint32_t it, done;
};

static inline void mw_strips(uint64_t rows, uint32_t cap, uint32_t* chunks, uint32_t* per, uint32_t* strips)
{
    *chunks = cdiv(rows, D3P_MW_LANES);
    *per = *chunks ? cdiv(*chunks, cap) : 0;
    *strips = *chunks ? cdiv(*chunks, *per) : 0;
}

// The workspaces are sized for min(chunks, cap) strips, which is monotone in rows (the strip count itself is not: 512 chunks are 512
// strips, 513 chunks 257) and never less than the strip count.
static inline uint32_t mw_strips_most(uint64_t rows, uint32_t cap)
{
    const uint64_t chunks = (rows + D3P_MW_LANES - 1) / D3P_MW_LANES;
    return chunks < cap ? (uint32_t)chunks : cap;
}

// the 256 lanes' sums of V values, red[v][lane], merged in one fixed tree; the result is red[v][0]
template <int V>
__device__ __forceinline__ void mw_tree(double (*red)[D3P_MW_LANES], int tid)
{
    for (int s = D3P_MW_LANES / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) {
#pragma unroll
            for (int v = 0; v < V; ++v) red[v][tid] += red[v][tid + s];
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(64) k_stack_init(StackState* st, uint32_t M)
{
    const uint32_t t = threadIdx.x;
    if (t < D3P_MW_MAX_M) st->w[t] = t < M ? 1.0 / (double)M : 0.0;
    if (t == 0) { st->it = 0u; st->done = 0u; }
}

template <int MT>
__global__ void __launch_bounds__(D3P_MW_LANES) k_stack_strip(const float* __restrict__ e, int64_t ld, uint64_t rows, uint32_t M, uint32_t per,
                                                               const StackState* st, double* part)
{
    __shared__ double red[MT + 1][D3P_MW_LANES];
    if (st->done) return;   // (uniform: every lane reads the same word)
    const int tid = threadIdx.x;
    double w[MT], acc[MT + 1];
#pragma unroll
    for (int m = 0; m < MT; ++m) w[m] = (uint32_t)m < M ? st->w[m] : 0.0;
#pragma unroll
    for (int v = 0; v <= MT; ++v) acc[v] = 0.0;
    const uint64_t r_lo = (uint64_t)blockIdx.x * per * D3P_MW_LANES + tid;
    for (uint32_t c = 0; c < per; ++c) {
        const uint64_t r = r_lo + (uint64_t)c * D3P_MW_LANES;
        if (r >= rows) break;
        double p[MT];
        double mx = -INFINITY;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            p[m] = (uint32_t)m < M ? (double)e[(size_t)m * ld + r] : -INFINITY;
            mx = p[m] > mx ? p[m] : mx;   // (a NaN never becomes mx; its own e - mx is NaN)
        }
        double den = 0.0;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if ((uint32_t)m < M) {
                p[m] = exp(p[m] - mx);
                den = fma(w[m], p[m], den);
            }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
            if ((uint32_t)m < M) acc[m] += p[m] / den;
        acc[MT] += mx + log(den);
    }
#pragma unroll
    for (int v = 0; v <= MT; ++v) red[v][tid] = acc[v];
    mw_tree<MT + 1>(red, tid);
    if ((uint32_t)tid <= M) part[(size_t)blockIdx.x * (M + 1) + tid] = (uint32_t)tid < M ? red[tid][0] : red[MT][0];
}

// The strips' partials come through LDS a tile of D3P_STACK_MERGE_TILE strips at a time: all 256 lanes load the tile (contiguous in
// part, every load in flight at once), then thread v <= M adds its column of the tile in ascending strip order.  The order of the
// additions is the plain loop's; a thread that walked part itself would wait for one dependent global load per strip.
__global__ void __launch_bounds__(D3P_MW_LANES) k_stack_merge(StackState* st, const double* part, uint32_t strips, uint32_t M, uint64_t rows,
                                                              double tol, uint32_t max_iter, double* w_out, double* info_out)
{
    __shared__ double tile[D3P_STACK_MERGE_TILE * (D3P_MW_MAX_M + 1)];
    __shared__ double sums[D3P_MW_MAX_M + 1];
    if (st->done) return;
    const uint32_t t = threadIdx.x, V = M + 1;
    double a = 0.0;
    for (uint32_t s0 = 0; s0 < strips; s0 += D3P_STACK_MERGE_TILE) {
        const uint32_t ns = strips - s0 < D3P_STACK_MERGE_TILE ? strips - s0 : D3P_STACK_MERGE_TILE;
        __syncthreads();   // the previous tile's readers are through
        for (uint32_t i = t; i < ns * V; i += D3P_MW_LANES) tile[i] = part[(size_t)s0 * V + i];
        __syncthreads();
        if (t <= M) {
            uint32_t k = 0;
            if (s0 == 0) {   // from strip 0's partial, not from 0.0
                a = tile[t];
                k = 1;
            }
            for (; k < ns; ++k) a += tile[k * V + t];
        }
    }
    if (t <= M) sums[t] = t < M ? a / (double)rows : a;
    __syncthreads();
    if (t != 0) return;
    double gmax = sums[0];
    bool nan = false;
    for (uint32_t m = 0; m < M; ++m) {
        nan |= sums[m] != sums[m];
        gmax = sums[m] > gmax ? sums[m] : gmax;
    }
    const double gap = nan ? __builtin_nan("") : gmax - 1.0;
    const uint32_t it = st->it;
    const bool converged = gap <= tol;   // (false for a NaN)
    if (converged || nan || it >= max_iter) {
        for (uint32_t m = 0; m < M; ++m) w_out[m] = nan ? gap : st->w[m];
        info_out[0] = (double)it;
        info_out[1] = converged ? 1.0 : 0.0;
        info_out[2] = gap;
        info_out[3] = nan ? gap : sums[M];
        st->done = 1u;
        return;
    }
    for (uint32_t m = 0; m < M; ++m) st->w[m] = st->w[m] * sums[m];
    st->it = it + 1u;
}

struct BbArgs {
    const float* e;
    int64_t ld;
    uint64_t rows;
    uint32_t M, B, per, chunks;
    const uint32_t* key;   // the threefry key, 2 words
    double* part;      // [strips][M + 1][B]
};

// -log(1 - u) for the float32 uniform of one threefry word (file comment: the float64 log of the exact float32 1 - u)
__device__ __forceinline__ double bb_weight(uint32_t bits)
{
    const float u = bits_to_uniform(bits, 0.0f, 1.0f);
    return -log((double)(1.0f - u));
}

template <int MT>
__global__ void __launch_bounds__(D3P_MW_LANES) k_bb_sums(BbArgs a)
{
    __shared__ double es[MT][D3P_MW_LANES];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const uint32_t b = blockIdx.y * D3P_MW_LANES + tid;
    const bool active = b < a.B;
    const uint32_t k0 = a.key[0], k1 = a.key[1];
    if (tid == 0) s_bad = 0;
    double S = 0.0, T[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) T[m] = 0.0;
    const uint32_t c_lo = blockIdx.x * a.per;
    const uint32_t c_hi = c_lo + a.per < a.chunks ? c_lo + a.per : a.chunks;
    for (uint32_t c = c_lo; c < c_hi; ++c) {
        const uint64_t r0 = (uint64_t)c * D3P_MW_LANES;
        const uint64_t left = a.rows - r0;   // >= 1
        const int n = left >= D3P_MW_LANES ? D3P_MW_LANES : (int)left;
        __syncthreads();   // the previous chunk's readers are through (and s_bad = 0 is in place)
        {
            bool bad = false, any = false;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                double v = 0.0;
                if ((uint32_t)m < a.M && tid < n) {
                    v = (double)a.e[(size_t)m * a.ld + r0 + tid];
                    bad |= !(v < INFINITY);   // NaN or +inf
                    any |= v > -INFINITY;
                }
                es[m][tid] = v;
            }
            if (tid < n && (bad || !any)) s_bad = 1;
        }
        __syncthreads();
        if (active) {
            for (int j = 0; j < n; j += 2) {
                uint32_t o0, o1;
                threefry2x32(k0, k1, (uint32_t)((r0 + j) >> 1), b, o0, o1);
                {
                    const double g = bb_weight(o0);
                    S += g;
#pragma unroll
                    for (int m = 0; m < MT; ++m) T[m] = fma(g, g == 0.0 ? 0.0 : es[m][j], T[m]);
                }
                if (j + 1 < n) {
                    const double g = bb_weight(o1);
                    S += g;
#pragma unroll
                    for (int m = 0; m < MT; ++m) T[m] = fma(g, g == 0.0 ? 0.0 : es[m][j + 1], T[m]);
                }
            }
        }
    }
    __syncthreads();
    if (!active) return;
    if (s_bad) S = __builtin_nan("");
    double* out = a.part + (size_t)blockIdx.x * (a.M + 1) * a.B + b;
    out[0] = S;
#pragma unroll
    for (int m = 0; m < MT; ++m)
        if ((uint32_t)m < a.M) out[(size_t)(1 + m) * a.B] = T[m];
}

template <int MT>
__global__ void __launch_bounds__(D3P_MW_LANES) k_bb_replicate(const double* part, uint32_t strips, uint32_t M, uint32_t B, uint64_t rows,
                                                                double* z_out, double* wb)
{
    const uint32_t b = blockIdx.x * D3P_MW_LANES + threadIdx.x;
    if (b >= B) return;
    const size_t step = (size_t)(M + 1) * B;
    double S = part[b], z[MT];
    for (uint32_t k = 1; k < strips; ++k) S += part[k * step + b];
    double mx = -INFINITY;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        z[m] = -INFINITY;
        if ((uint32_t)m < M) {
            const double* p = part + (size_t)(1 + m) * B + b;
            double T = p[0];
            for (uint32_t k = 1; k < strips; ++k) T += p[k * step];
            z[m] = ((double)rows * T) / S;
            z_out[(size_t)b * M + m] = z[m];
            mx = z[m] > mx ? z[m] : mx;
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if ((uint32_t)m < M) {
            z[m] = exp(z[m] - mx);   // a NaN z, or -inf in every model (mx = -inf): NaN, and through the sum every weight
            sum += z[m];
        }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
        if ((uint32_t)m < M) wb[(size_t)m * B + b] = z[m] / sum;
}

__global__ void __launch_bounds__(D3P_MW_LANES) k_bb_mean(const double* wb, uint32_t B, double* w_out)
{
    __shared__ double red[1][D3P_MW_LANES];
    const int tid = threadIdx.x;
    const double* p = wb + (size_t)blockIdx.x * B;
    double a = 0.0;
    for (uint32_t b = tid; b < B; b += D3P_MW_LANES) a += p[b];
    red[0][tid] = a;
    mw_tree<1>(red, tid);
    if (tid == 0) w_out[blockIdx.x] = red[0][0] / (double)B;
}

static int g_stack_chunk = D3P_STACK_DEFAULT_CHUNK;

// the checks both entries share, in the order the header lists them; the device question comes last
static int mw_check(const char* what, const float* e, int64_t ld, uint64_t rows, uint32_t M, const void* out_a, const void* out_b,
                    const void* ws)
{
    if (!e || !out_a || !out_b || !ws) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((uintptr_t)e & 3u) return fail(D3P_E_INVALID_ARG, "%s: e is not aligned to 4 bytes", what);
    if (((uintptr_t)out_a | (uintptr_t)out_b | (uintptr_t)ws) & 7u)
        return fail(D3P_E_INVALID_ARG, "%s: the outputs and the workspace must be aligned to 8 bytes", what);
    if (M < 1 || M > D3P_MW_MAX_M) return fail(D3P_E_INVALID_ARG, "%s: 1 <= M <= %d models are required, got %u", what, D3P_MW_MAX_M, M);
    if (rows < 1) return fail(D3P_E_INVALID_ARG, "%s: rows >= 1 is required", what);
    if (ld < 0 || (uint64_t)ld < rows) return fail(D3P_E_INVALID_ARG, "%s: ld >= rows is required", what);
    return D3P_OK;
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_stacking_strip_rows(void) { return D3P_MW_LANES; }

uint32_t d3p_bb_pseudo_bma_strip_rows(void) { return D3P_MW_LANES; }

int d3p_stacking_set_chunk(int32_t n)
{
    if (n != 0 && n < 64) return fail(D3P_E_INVALID_ARG, "d3p_stacking_set_chunk: a chunk of at least 64 evaluations (or 0: the default), got %d", n);
    const int before = g_stack_chunk;
    g_stack_chunk = n ? n : D3P_STACK_DEFAULT_CHUNK;
    return before;
}

size_t d3p_stacking_workspace(uint64_t rows, uint32_t M)
{
    return sizeof(StackState) + (size_t)mw_strips_most(rows, D3P_STACK_MAX_STRIPS) * (M + 1) * sizeof(double);
}

int d3p_stacking_weights(void* stream, const float* e_dev, int64_t ld, uint64_t rows, uint32_t M, double tol, uint32_t max_iter,
                         double* w_out_dev, double* info_out_dev, void* workspace_dev, size_t workspace_bytes)
{
    const char* what = "d3p_stacking_weights";
    if (int rc = mw_check(what, e_dev, ld, rows, M, w_out_dev, info_out_dev, workspace_dev)) return rc;
    if (!(tol > 0.0)) return fail(D3P_E_INVALID_ARG, "%s: tol > 0 is required", what);
    if (max_iter < 1) return fail(D3P_E_INVALID_ARG, "%s: max_iter >= 1 is required", what);
    if (rows > 0xffffffffull) return fail(D3P_E_UNSUPPORTED, "%s: rows <= 2^32 - 1 is served", what);
    const size_t need = d3p_stacking_workspace(rows, M);
    if (workspace_bytes < need) return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace_bytes, need);
    if (!is_device_ptr(e_dev) || !is_device_ptr(w_out_dev) || !is_device_ptr(info_out_dev) || !is_device_ptr(workspace_dev))
        return fail(D3P_E_INVALID_ARG, "%s: e, the outputs and the workspace must be device memory", what);
    hipStream_t s = (hipStream_t)stream;
    uint32_t chunks, per, strips;
    mw_strips(rows, D3P_STACK_MAX_STRIPS, &chunks, &per, &strips);
    StackState* st = static_cast<StackState*>(workspace_dev);
    double* part = reinterpret_cast<double*>(st + 1);
    hipLaunchKernelGGL(k_stack_init, dim3(1), dim3(64), 0, s, st, M);
    if (int rc = check_launch(what)) return rc;
    const uint64_t total = (uint64_t)max_iter + 1;   // evaluations 0 .. max_iter
    const uint32_t chunk = (uint32_t)g_stack_chunk;
    for (uint64_t at = 0; at < total;) {
        const uint64_t upto = at + chunk < total ? at + chunk : total;
        for (; at < upto; ++at) {
            if (M <= 4) hipLaunchKernelGGL((k_stack_strip<4>), dim3(strips), dim3(D3P_MW_LANES), 0, s, e_dev, ld, rows, M, per, st, part);
            else hipLaunchKernelGGL((k_stack_strip<16>), dim3(strips), dim3(D3P_MW_LANES), 0, s, e_dev, ld, rows, M, per, st, part);
            hipLaunchKernelGGL(k_stack_merge, dim3(1), dim3(D3P_MW_LANES), 0, s, st, part, strips, M, rows, tol, max_iter, w_out_dev, info_out_dev);
        }
        if (int rc = check_launch(what)) return rc;
        uint32_t done = 0;
        D3P_HIP_TRY(hipMemcpyAsync(&done, &st->done, sizeof(done), hipMemcpyDeviceToHost, s));
        D3P_HIP_TRY(hipStreamSynchronize(s));
        if (done) return D3P_OK;
    }
    return fail(D3P_E_HIP, "%s: the run did not stop within max_iter + 1 evaluations", what);   // (not reachable: evaluation max_iter stops)
}

size_t d3p_bb_pseudo_bma_workspace(uint64_t rows, uint32_t M, uint32_t B)
{
    return ((size_t)mw_strips_most(rows, D3P_BB_MAX_STRIPS) * (M + 1) + M) * B * sizeof(double);
}

int d3p_bb_pseudo_bma(void* stream, const uint32_t* key_dev, const float* e_dev, int64_t ld, uint64_t rows, uint32_t M, uint32_t B,
                      double* w_out_dev, double* z_out_dev, void* workspace_dev, size_t workspace_bytes)
{
    const char* what = "d3p_bb_pseudo_bma";
    if (!key_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((uintptr_t)key_dev & 3u) return fail(D3P_E_INVALID_ARG, "%s: the key is not aligned to 4 bytes", what);
    if (int rc = mw_check(what, e_dev, ld, rows, M, w_out_dev, z_out_dev, workspace_dev)) return rc;
    if (B < 1 || B > 65535) return fail(D3P_E_INVALID_ARG, "%s: 1 <= B <= 65535 replicates are required, got %u", what, B);
    if (rows > 0xffffffffull) return fail(D3P_E_UNSUPPORTED, "%s: rows <= 2^32 - 1 is served", what);
    const size_t need = d3p_bb_pseudo_bma_workspace(rows, M, B);
    if (workspace_bytes < need) return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace_bytes, need);
    if (!is_device_ptr(key_dev) || !is_device_ptr(e_dev) || !is_device_ptr(w_out_dev) || !is_device_ptr(z_out_dev) || !is_device_ptr(workspace_dev))
        return fail(D3P_E_INVALID_ARG, "%s: the key, e, the outputs and the workspace must be device memory", what);
    hipStream_t s = (hipStream_t)stream;
    BbArgs a;
    uint32_t strips;
    mw_strips(rows, D3P_BB_MAX_STRIPS, &a.chunks, &a.per, &strips);
    a.e = e_dev; a.ld = ld; a.rows = rows; a.M = M; a.B = B; a.key = key_dev;
    a.part = static_cast<double*>(workspace_dev);
    double* wb = a.part + (size_t)mw_strips_most(rows, D3P_BB_MAX_STRIPS) * (M + 1) * B;
    const dim3 grid(strips, cdiv(B, D3P_MW_LANES));
    if (M <= 4) hipLaunchKernelGGL((k_bb_sums<4>), grid, dim3(D3P_MW_LANES), 0, s, a);
    else hipLaunchKernelGGL((k_bb_sums<16>), grid, dim3(D3P_MW_LANES), 0, s, a);
    if (int rc = check_launch(what)) return rc;
    if (M <= 4)
        hipLaunchKernelGGL((k_bb_replicate<4>), dim3(cdiv(B, D3P_MW_LANES)), dim3(D3P_MW_LANES), 0, s, a.part, strips, M, B, rows, z_out_dev, wb);
    else
        hipLaunchKernelGGL((k_bb_replicate<16>), dim3(cdiv(B, D3P_MW_LANES)), dim3(D3P_MW_LANES), 0, s, a.part, strips, M, B, rows, z_out_dev, wb);
    if (int rc = check_launch(what)) return rc;
    hipLaunchKernelGGL(k_bb_mean, dim3(M), dim3(D3P_MW_LANES), 0, s, wb, B, w_out_dev);
    return check_launch(what);
}

}  // extern "C"
