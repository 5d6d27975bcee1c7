// Held-out log predictive density and responsibilities of the Gaussian mixture model over n posterior draws
// (d3p_amd/mixture_density.py).  The latents are the packed rows d3p_predict_gmm_draws writes: draw s is
// [pis (k) | mus (k d) | sigs (k d)] at latent + s latent_ld.  With
//   a[s, r, j] = log pis[s, j] + sum_c ( -((x[r, c] - mus[s, j, c]) / sigs[s, j, c])^2 / 2 - log sigs[s, j, c] - log(2 pi) / 2 )
// the outputs are
//   rows form     ll[s, r]   = logsumexp_j a[s, r, j]                                 (n x rows)
//   reduced form  lppd[r]    = logsumexp_s ll[s, r] - log n                           (rows)
//                 resp[r, j] = (1 / n) sum_s exp(a[s, r, j] - ll[s, r])               (rows x k)
//   WAIC form     lppd[r]    = the reduced form's value, bit for bit                  (rows)
//                 pwaic[r]   = Var_s ll[s, r] = M2 / (n - ddof)                       (rows)
// The reduced form writes neither a nor ll to memory.
//
// Geometry.  A workgroup owns D3P_GD_ROW_TILE = 64 rows, staged once in LDS with an odd stride (d | 1: the 32 lanes of a bank group
// read 32 different banks), and walks all n draws: obs is read from memory once.  Lane l of every wave owns row l.  The workgroup's W
// waves split the draws: wave w takes the draws s = w, w + W, w + 2 W, ... in that order.  W = D3P_GD_DRAW_TILE = 4; only where the
// staged latents of four draws do not fit beside the row tile (k d > 3584 or so: the two largest shapes) W = 2.  W depends on (k, d)
// alone, never on rows, n or the grid.
//
// Per draw a wave stages its own copy of the draw in LDS as pairs (mus, 1 / sigs) -- the reciprocal is formed ONCE per draw, a term is
// t = x - mu; z = t rinv; q += z z -- and hoists, per component, C_j = (logf(pis_j) - H_j) - fl(d) log(2 pi) / 2 with H_j = sum_c
// logf(sigs_jc) taken in index order in float32 (the logs go through LDS transposed, so that lane j sums component j without a bank
// conflict).  Then a_j = -0.5 q_j + C_j, every operation rounded on its own (fp contract off): tests/mixture_density_ref.py restates
// exactly this order.  The DIRECT form, as k_gmm_assign's comment explains: vector float32, not a matrix product.  The pair reads are
// wave-uniform addresses (LDS broadcasts, one ds_read_b64 per term); a lane's sum over c runs in index order with no cross-lane step.
//
// ll = m + logf(sum_j expf(a_j - m)), m = max_j a_j, the sum in index order; a draw's responsibility of j is expf(a_j - m) * (1 / sum).
// Per row a wave keeps a running (max, sum) of ll exactly as k_loglik's lppd form does (one expf per draw, the sum in float64) and k
// float64 responsibility sums in registers (KMAX = 4 / 16 / 32).  At the end the waves hand their accumulators to wave 0 through LDS,
// wave 1 first, then 2, then 3: a fixed order, no atomics, bit-identical between calls.
//
// Special values: pis_j = 0 gives a_j = -inf, which adds nothing; a draw whose every a_j is -inf has ll = -inf (never NaN) and
// contributes NaN (0 / 0) to the row's resp; every draw -inf gives lppd = -inf.  A NaN in a row of obs or in a draw's latents makes
// every a_j of that (draw, row) NaN in effect: ll is NaN and so is every responsibility, as d3p_gmm_assign makes the whole row NaN.
//
// The WAIC form (REDUCE = 2; d3p_amd/criteria.py) keeps no responsibility sums: per row the running (max, sum)
// as the reduced form, and beside it k_moments' shifted sums of ll (d3p_shifted_sums.h): c = the wave's first finite ll of the row,
// float64 sums of (ll - c) and (ll - c)^2, a count and flags.  Wave 0 merges the waves' parts in Chan's pairwise form in the same
// fixed order 1, 2, 3 (a wave that owned no draw has count 0 and is skipped, never divided by) and finishes pwaic = M2 / (n - ddof)
// in float64, rounded to float32 once; every draw of a row equal gives exactly 0.  Special values as k_loglik's WAIC form: ll = -inf
// is not added but remembered, and such a row gets pwaic = +inf (also when every draw is -inf, where lppd = -inf); a NaN ll makes
// both outputs NaN; ll = +inf (not reached from finite inputs) is not added either and makes pwaic NaN.
//
// The draw-sums form (REDUCE = 3; d3p_amd/mixture_diagnostics.py): out[s] = sum_{r < rows} ll[s, r] as float64,
// every other reduction here runs over the draws, once per row; this one runs over the rows, once per draw.  ll[s, r] is bit for bit
// the float32 value the rows form writes: the same instantiated text up to the line that stores it.  Grid: the table's row tiles are
// cut into strips of `per` consecutive tiles,
//   tiles = ceil(rows / 64);  per = ceil(tiles / 2048);  strips = ceil(tiles / per)  (<= 2048)
// a function of rows alone: d3p_draw_sums.hip's row_strips (d3p_row_sums.h) at this file's tile and cap.  A workgroup walks the tiles
// of its strip in ascending order and, per tile, all n draws exactly as the other forms do (the same W, the same staging).
// Summation order of out[s], fixed:
//   tile sum   = the 64 lanes' (double)ll in the xor butterfly v = v + v[lane ^ off], off = 1, 2, 4, 8, 16, 32, i.e. the balanced binary
//                tree over the rows of the tile in index order; a row past the end is exactly 0.0 (its value, of a staged zero row, is
//                computed and dropped);
//   strip sum  = the tile sums of the strip added one by one in ascending tile order, from 0.0, kept at ws[strip][s] by the lane
//                that owns (strip, s) -- lane 0 of wave s % W of workgroup `strip`, always the same -- with a plain load, add and store;
//   out[s]     = the strip sums added in ascending strip order, starting from strip 0's (k_strip_merge<1, -1, -1>, a second launch).
// No floating-point atomics, no arrival order; a draw's sum does not depend on the other draws of the launch.  Nothing is clamped:
// a draw with ll = -inf in some row sums to -inf, a NaN row of obs makes every draw NaN, a NaN in a draw's latents that draw only.
#include "d3p_colreduce.h"
#include "d3p_device.h"
#include "d3p_row_sums.h"
#include "d3p_shifted_sums.h"

namespace d3p {

#define D3P_GD_ROW_TILE 64
#define D3P_GD_DRAW_TILE 4
#define D3P_GD_LDS_MAX 163840   // 160 KiB: a compute unit's LDS
#define D3P_GD_MAX_STRIPS 2048  // draw-sums form: workgroups of one launch (several per compute unit: the kernel is latency-bound)

struct GmmDensityArgs {
    const float* obs;
    const float* lat;
    int64_t ld;
    uint32_t rows, n;
    int k, d;
    float* ll;     // rows form
    float* lppd;   // reduced form, nullable
    float* resp;   // reduced form, nullable
    float* pwaic;    // WAIC form (with lppd; both required)
    uint32_t ddof;   // WAIC form: 0 or 1
    double* part;    // draw-sums form: [strip][n], a strip's running sums (the workspace)
    uint32_t tiles;  //                 row tiles of the table
    uint32_t per;    //                 row tiles per strip
};

// floats of LDS in front of the waves' latent copies (the row tile, rounded up to a float2 boundary) and per wave
__host__ __device__ inline int gd_tile_floats(int d) { return (D3P_GD_ROW_TILE * (d | 1) + 1) & ~1; }
__host__ __device__ inline int gd_wave_floats(int k, int d) { return 2 * k * d + ((k + 1) & ~1); }

template <int KMAX, int REDUCE>
__global__ void __launch_bounds__(256) k_gmm_density(GmmDensityArgs g)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = (int)(blockDim.x >> 6);
    const int k = g.k, d = g.d, kd = k * d, ldx = d | 1;
    float* xs = lds;
    float* mine = lds + gd_tile_floats(d) + wave * gd_wave_floats(k, d);
    float2* st = reinterpret_cast<float2*>(mine);   // [j d + c] = (mus, 1 / sigs)
    float* lg = mine;                               // [c k + j] = logf(sigs): the same floats, before the pairs are written
    float* cj = mine + 2 * kd;                      // [j] = C_j
    // REDUCE == 3 walks the row tiles of its strip in ascending order; every other form owns the one tile of its workgroup (the loop's
    // condition is false at compile time and its body, left at its indentation, is the text those forms always had)
    uint32_t tile_lo = blockIdx.x, tile_hi = tile_lo + 1;
    if (REDUCE == 3) strip_tiles(g.per, g.tiles, tile_lo, tile_hi);
    uint32_t tile = tile_lo;
    bool live;
    float run_m = -INFINITY;
    double run_s = 0.0;
    double racc[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) racc[j] = 0.0;
    double v1 = 0.0, v2 = 0.0;        // WAIC form: sum (ll - vc), sum (ll - vc)^2
    float vc = 0.f;                   //            the shift: this wave's first finite ll of the row
    uint32_t vcnt = 0, vflags = 0;    //            values in the sums; D3P_SHIFTED_* flags
    do {
    const uint64_t r0 = (uint64_t)tile * D3P_GD_ROW_TILE;
    const uint32_t left = g.rows - (uint32_t)r0;
    const uint32_t total = (left < D3P_GD_ROW_TILE ? left : D3P_GD_ROW_TILE) * (uint32_t)d;
    for (uint32_t e = tid; e < (uint32_t)(D3P_GD_ROW_TILE * d); e += blockDim.x) {
        const uint32_t row = e / (uint32_t)d, c = e - row * (uint32_t)d;
        xs[row * ldx + c] = e < total ? g.obs[r0 * (uint64_t)d + e] : 0.f;   // (rows past the end: zeros, never written out)
    }
    live = r0 + lane < g.rows;
    const float* xrow = xs + lane * ldx;
    // every wave runs the same number of passes (the barriers are workgroup-wide); a wave without a draw in the last pass idles
    const uint32_t passes = (g.n + (uint32_t)W - 1) / (uint32_t)W;
    for (uint32_t it = 0; it < passes; ++it) {
        const uint32_t s = it * (uint32_t)W + (uint32_t)wave;
        const bool active = s < g.n;
        const float* row = g.lat + (size_t)s * (size_t)g.ld;
        __syncthreads();   // the previous draw's pairs are read (first pass: the row tile is staged)
        if (active)
            for (int j = 0; j < k; ++j)
                for (int c = lane; c < d; c += 64) lg[c * k + j] = logf(row[k + kd + j * d + c]);
        __syncthreads();
        float C = 0.f;
        if (active && lane < k) {
            float H = 0.f;
            for (int c = 0; c < d; ++c) H = H + lg[c * k + lane];   // index order
            C = (logf(row[lane]) - H) - (float)d * D3P_HALF_LOG_2PI;
        }
        __syncthreads();   // the logs are read before the pairs overwrite them
        if (active) {
            if (lane < k) cj[lane] = C;
            for (int j = 0; j < k; ++j)
                for (int c = lane; c < d; c += 64) st[j * d + c] = make_float2(row[k + j * d + c], 1.0f / row[k + kd + j * d + c]);
        }
        __syncthreads();
        // (no barrier below this line inside the loop; the draw-sums form keeps the lanes past the end for its butterfly: their rows
        // are staged zeros, their values are computed and dropped)
        if (REDUCE == 3 ? !active : !(active && live)) continue;
        double prev = 0.0;   // draw-sums form: the strip's running sum of this draw, asked for before the evaluation that hides the load
        if (REDUCE == 3 && lane == 0 && tile != tile_lo) prev = g.part[(size_t)blockIdx.x * g.n + s];
        float q[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) q[j] = 0.f;
        for (int c = 0; c < d; ++c) {
            const float xv = xrow[c];
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                if (j < k) {
                    const float2 p = st[j * d + c];
                    const float t = xv - p.x;
                    const float z = t * p.y;
                    q[j] = q[j] + z * z;
                }
            }
        }
        float m = -INFINITY;
        bool nan = false;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j < k) {
                const float a = -0.5f * q[j] + cj[j];
                q[j] = a;
                nan |= a != a;
                m = a > m ? a : m;
            }
        }
        float ll, rinv;
        if (nan || m == -INFINITY) {
            // a NaN anywhere: the whole (draw, row) is NaN; every component -inf: ll = -inf and the responsibilities are 0 / 0
            ll = nan ? __builtin_nanf("") : -INFINITY;
            rinv = __builtin_nanf("");
#pragma unroll
            for (int j = 0; j < KMAX; ++j) q[j] = 1.f;
        } else {
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                if (j < k) {
                    const float e = expf(q[j] - m);
                    q[j] = e;
                    sum = sum + e;   // index order
                }
            }
            ll = m + logf(sum);
            rinv = 1.0f / sum;
        }
        if (!REDUCE) {
            g.ll[(size_t)s * g.rows + (r0 + lane)] = ll;
        } else if (REDUCE == 3) {
            // the tile's 64 values of this draw in a fixed tree: a lane past the end gives exactly 0.0; after the six steps every lane
            // holds the same float64 sum (IEEE addition commutes).  Lane 0 of the wave that owns the draw -- always this one -- adds
            // it to the strip's running sum by a plain load, add and store in program order.
            double v = live ? (double)ll : 0.0;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off);
            if (lane == 0) g.part[(size_t)blockIdx.x * g.n + s] = prev + v;
        } else {
            // k_loglik's running (max, sum): one expf per draw, the sum in float64
            if (ll > run_m) {
                run_s = run_s * (double)expf(run_m - ll) + 1.0;
                run_m = ll;
            } else if (ll != -INFINITY) {   // (a NaN ll makes the sum NaN)
                run_s += (double)expf(ll - run_m);
            }
            if (REDUCE == 1 && g.resp) {
#pragma unroll
                for (int j = 0; j < KMAX; ++j)
                    if (j < k) racc[j] += (double)(q[j] * rinv);
            }
            if (REDUCE == 2) shifted_add(ll, vc, v1, v2, vcnt, vflags);
        }
    }
    if (REDUCE == 3) __syncthreads();   // the tile's rows are read before the next tile overwrites them
    } while (REDUCE == 3 && ++tile < tile_hi);
    if (REDUCE == 1 || REDUCE == 2) {
        // waves 1 .. W - 1 hand their accumulators to wave 0, one after the other; the row tile and the latents are no longer needed
        double* Rs = reinterpret_cast<double*>(lds);   // [j][lane]
        double* Ss = Rs + (REDUCE == 2 ? 0 : (size_t)k * 64);   // [lane] (the WAIC form has no Rs)
        float* Ms = reinterpret_cast<float*>(Ss + 64);  // [lane]
        // WAIC form, behind them: [2][lane] shifted sums, then [lane] shifts, counts and flags
        double* Vs = reinterpret_cast<double*>(Ms + 64);
        float* Cs = reinterpret_cast<float*>(Vs + 128);
        uint32_t* Ks = reinterpret_cast<uint32_t*>(Cs + 64);
        uint32_t* Fs = Ks + 64;
        uint32_t ka = vcnt;
        double ma = 0.0, qa = 0.0;
        if (REDUCE == 2 && ka) moments_part(ka, vc, v1, v2, ma, qa);   // wave 0's own part first
        __syncthreads();
        for (int w = 1; w < W; ++w) {
            if (wave == w) {
                Ss[lane] = run_s;
                Ms[lane] = run_m;
                if (REDUCE == 2) { Vs[lane] = v1; Vs[64 + lane] = v2; Cs[lane] = vc; Ks[lane] = vcnt; Fs[lane] = vflags; }
#pragma unroll
                for (int j = 0; j < KMAX; ++j)
                    if (REDUCE == 1 && j < k) Rs[j * 64 + lane] = racc[j];
            }
            __syncthreads();
            if (wave == 0) {
                const double s1 = Ss[lane];
                const float m1 = Ms[lane];
                const float mm = fmaxf(run_m, m1);
                // a wave that saw no finite value has sum 0 -- or NaN, if a NaN came by: it is taken as it is, so a NaN stays
                const double a0 = run_m == -INFINITY ? run_s : run_s * exp((double)run_m - (double)mm);
                const double a1 = m1 == -INFINITY ? s1 : s1 * exp((double)m1 - (double)mm);
                run_s = a0 + a1;
                run_m = mm;
#pragma unroll
                for (int j = 0; j < KMAX; ++j)
                    if (REDUCE == 1 && j < k) racc[j] += Rs[j * 64 + lane];
                if (REDUCE == 2) {
                    const uint32_t kb = Ks[lane];
                    double mb = 0.0, qb = 0.0;
                    if (kb) moments_part(kb, Cs[lane], Vs[lane], Vs[64 + lane], mb, qb);
                    chan_merge(ka, ma, qa, kb, mb, qb);
                    vflags |= Fs[lane];
                }
            }
            __syncthreads();
        }
        if (wave == 0 && live) {
            const uint64_t r = (uint64_t)tile_lo * D3P_GD_ROW_TILE + lane;
            if (g.lppd)
                g.lppd[r] = (run_m == -INFINITY && run_s == 0.0) ? -INFINITY : (float)(((double)run_m + log(run_s)) - log((double)g.n));
            if (REDUCE == 1 && g.resp) {
#pragma unroll
                for (int j = 0; j < KMAX; ++j)
                    if (j < k) g.resp[r * (uint64_t)k + j] = (float)(racc[j] / (double)g.n);
            }
            if (REDUCE == 2) g.pwaic[r] = pwaic_value(qa, g.n, g.ddof, vflags);   // (no finite ll at all: M2 = 0, and the flags say so)
        }
    }
}

// four waves split the draws where their four latent copies fit beside the row tile, otherwise two: a function of (k, d) alone.
// Returns the bytes of LDS of the staging.
static size_t gd_waves(int k, int d, int* W)
{
    *W = D3P_GD_DRAW_TILE;
    size_t lds = sizeof(float) * ((size_t)gd_tile_floats(d) + (size_t)*W * gd_wave_floats(k, d));
    if (lds > D3P_GD_LDS_MAX) {
        *W = 2;
        lds = sizeof(float) * ((size_t)gd_tile_floats(d) + (size_t)*W * gd_wave_floats(k, d));
    }
    return lds;
}

template <int KMAX, int REDUCE>
static int gd_launch(const char* what, hipStream_t s, const GmmDensityArgs& g, int W, size_t lds, uint32_t grid)
{
    const void* fn = reinterpret_cast<const void*>(&k_gmm_density<KMAX, REDUCE>);
    if (int rc = dynamic_lds_opt_in(fn, D3P_GD_LDS_MAX, what)) return rc;
    hipLaunchKernelGGL((k_gmm_density<KMAX, REDUCE>), dim3(grid), dim3(64 * W), lds, s, g);
    return check_launch(what);
}

template <int REDUCE>
static int gd_entry(const char* what, void* stream, const float* obs, uint64_t rows, int32_t d, const float* latent, int64_t ld, int32_t k,
                    uint32_t n, float* ll, float* lppd, float* resp, float* pwaic = nullptr, uint32_t ddof = 0)
{
    if (!obs || !latent) return fail(D3P_E_INVALID_ARG, "%s: null obs / latent pointer", what);
    if (REDUCE == 2 && (!lppd || !pwaic)) return fail(D3P_E_INVALID_ARG, "%s: null lppd / pwaic pointer", what);
    if (REDUCE ? (!lppd && !resp) : !ll)
        return fail(D3P_E_INVALID_ARG, REDUCE ? "%s: at least one of the two outputs is required" : "%s: null output pointer", what);
    if (!aligned4(obs) || !aligned4(latent) || !aligned4(ll) || !aligned4(lppd) || !aligned4(resp) || !aligned4(pwaic))
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (k < 1 || d < 1) return fail(D3P_E_INVALID_ARG, "%s: k and d must be >= 1 (k = %d, d = %d)", what, k, d);
    if (k > 32 || d > 256 || (k > 16 && d > 128))
        return fail(D3P_E_UNSUPPORTED, "%s: supported shapes are k <= 16 with d <= 256 and k <= 32 with d <= 128 (k = %d, d = %d)", what, k, d);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n must be >= 1", what);
    if (n > 0x7fffffffu) return fail(D3P_E_UNSUPPORTED, "%s: n <= 2^31 - 1", what);
    if (REDUCE == 2 && ddof > 1) return fail(D3P_E_INVALID_ARG, "%s: ddof must be 0 or 1 (got %u)", what, ddof);
    if (REDUCE == 2 && n <= ddof) return fail(D3P_E_INVALID_ARG, "%s: n > ddof is required (n = %u, ddof = %u)", what, n, ddof);
    if (ld < (int64_t)k + 2 * (int64_t)k * d) return fail(D3P_E_INVALID_ARG, "%s: a latent row holds k + 2 k d values", what);
    if (rows > 0xFFFFFFFFull || rows * (uint64_t)d > 0xFFFFFFFFull) return fail(D3P_E_UNSUPPORTED, "%s: rows d < 2^32", what);
    if (rows == 0) return D3P_OK;
    if (!is_device_ptr(obs) || !is_device_ptr(latent) || (ll && !is_device_ptr(ll)) || (lppd && !is_device_ptr(lppd)) ||
        (resp && !is_device_ptr(resp)) || (pwaic && !is_device_ptr(pwaic)))
        return fail(D3P_E_INVALID_ARG, "%s: every pointer must be device memory", what);
    GmmDensityArgs g = {};
    g.obs = obs; g.lat = latent; g.ld = ld; g.rows = (uint32_t)rows; g.n = n; g.k = k; g.d = d; g.ll = ll; g.lppd = lppd; g.resp = resp;
    g.pwaic = pwaic; g.ddof = ddof;
    // (the WAIC form hands over the sum, the maximum, two shifted sums, the shift, the count and the flags per lane)
    const size_t combine = REDUCE == 2 ? (size_t)64 * (8 + 4 + 2 * 8 + 3 * 4) : REDUCE ? (size_t)64 * 8 * (k + 1) + 64 * 4 : 0;
    int W;
    size_t lds = gd_waves(k, d, &W);
    if (lds < combine) lds = combine;
    if (lds > D3P_GD_LDS_MAX) return fail(D3P_E_UNSUPPORTED, "%s: %zu bytes of LDS needed (k = %d, d = %d)", what, lds, k, d);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t grid = cdiv(g.rows, D3P_GD_ROW_TILE);
    if (k <= 4) return gd_launch<4, REDUCE>(what, s, g, W, lds, grid);
    if (k <= 16) return gd_launch<16, REDUCE>(what, s, g, W, lds, grid);
    return gd_launch<32, REDUCE>(what, s, g, W, lds, grid);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

int d3p_gmm_loglik_rows(void* stream, const float* obs_dev, uint64_t rows, int32_t d, const float* latent_dev, int64_t latent_ld, int32_t k,
                        uint32_t n, float* ll_out_dev)
{
    return gd_entry<0>("d3p_gmm_loglik_rows", stream, obs_dev, rows, d, latent_dev, latent_ld, k, n, ll_out_dev, nullptr, nullptr);
}

int d3p_gmm_loglik_reduce(void* stream, const float* obs_dev, uint64_t rows, int32_t d, const float* latent_dev, int64_t latent_ld, int32_t k,
                          uint32_t n, float* lppd_out_dev, float* resp_out_dev)
{
    return gd_entry<1>("d3p_gmm_loglik_reduce", stream, obs_dev, rows, d, latent_dev, latent_ld, k, n, nullptr, lppd_out_dev, resp_out_dev);
}

int d3p_gmm_loglik_waic(void* stream, const float* obs_dev, uint64_t rows, int32_t d, const float* latent_dev, int64_t latent_ld, int32_t k,
                        uint32_t n, uint32_t ddof, float* lppd_rows_dev, float* pwaic_rows_dev)
{
    return gd_entry<2>("d3p_gmm_loglik_waic", stream, obs_dev, rows, d, latent_dev, latent_ld, k, n, nullptr, lppd_rows_dev, nullptr, pwaic_rows_dev,
                       ddof);
}

size_t d3p_gmm_loglik_draw_sums_workspace(uint64_t rows, int32_t d, int32_t k, uint32_t n)
{
    (void)d; (void)k;   // (the strips are a function of rows alone)
    uint32_t tiles, per, strips;
    row_strips(rows, D3P_GD_ROW_TILE, D3P_GD_MAX_STRIPS, &tiles, &per, &strips);
    return (size_t)strips * n * sizeof(double);
}

int d3p_gmm_loglik_draw_sums(void* stream, const float* obs_dev, uint64_t rows, int32_t d, const float* latent_dev, int64_t latent_ld,
                             int32_t k, uint32_t n, double* out_dev, void* workspace_dev, size_t workspace_bytes)
{
    const char* what = "d3p_gmm_loglik_draw_sums";
    // gd_entry's checks in its order, then the output's and the workspace's; all of them before any launch
    if (!obs_dev || !latent_dev) return fail(D3P_E_INVALID_ARG, "%s: null obs / latent pointer", what);
    if (!out_dev) return fail(D3P_E_INVALID_ARG, "%s: null output pointer", what);
    if (!aligned4(obs_dev) || !aligned4(latent_dev)) return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (k < 1 || d < 1) return fail(D3P_E_INVALID_ARG, "%s: k and d must be >= 1 (k = %d, d = %d)", what, k, d);
    if (k > 32 || d > 256 || (k > 16 && d > 128))
        return fail(D3P_E_UNSUPPORTED, "%s: supported shapes are k <= 16 with d <= 256 and k <= 32 with d <= 128 (k = %d, d = %d)", what, k, d);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n must be >= 1", what);
    if (n > 0x7fffffffu) return fail(D3P_E_UNSUPPORTED, "%s: n <= 2^31 - 1", what);
    if (latent_ld < (int64_t)k + 2 * (int64_t)k * d) return fail(D3P_E_INVALID_ARG, "%s: a latent row holds k + 2 k d values", what);
    if (rows > 0xFFFFFFFFull || rows * (uint64_t)d > 0xFFFFFFFFull) return fail(D3P_E_UNSUPPORTED, "%s: rows d < 2^32", what);
    if ((uintptr_t)out_dev % sizeof(double)) return fail(D3P_E_INVALID_ARG, "%s: out must be aligned to 8 bytes", what);
    hipStream_t s = (hipStream_t)stream;
    if (rows == 0) {   // the empty sum, without a launch
        if (!is_device_ptr(out_dev)) return fail(D3P_E_INVALID_ARG, "%s: out must be device memory", what);
        D3P_HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)n * sizeof(double), s));
        return D3P_OK;
    }
    if (!is_device_ptr(obs_dev) || !is_device_ptr(latent_dev) || !is_device_ptr(out_dev))
        return fail(D3P_E_INVALID_ARG, "%s: every pointer must be device memory", what);
    GmmDensityArgs g = {};
    uint32_t strips;
    row_strips(rows, D3P_GD_ROW_TILE, D3P_GD_MAX_STRIPS, &g.tiles, &g.per, &strips);
    if (int rc = row_workspace_check(what, "d3p_gmm_loglik_draw_sums_workspace", workspace_dev, workspace_bytes, strips, 1, n)) return rc;
    g.obs = obs_dev; g.lat = latent_dev; g.ld = latent_ld; g.rows = (uint32_t)rows; g.n = n; g.k = k; g.d = d;
    g.part = static_cast<double*>(workspace_dev);
    int W;
    const size_t lds = gd_waves(k, d, &W);   // the other forms' rule: the same W, so the same staging per draw
    if (lds > D3P_GD_LDS_MAX) return fail(D3P_E_UNSUPPORTED, "%s: %zu bytes of LDS needed (k = %d, d = %d)", what, lds, k, d);
    if (int rc = k <= 4 ? gd_launch<4, 3>(what, s, g, W, lds, strips) : k <= 16 ? gd_launch<16, 3>(what, s, g, W, lds, strips)
                                                                                : gd_launch<32, 3>(what, s, g, W, lds, strips))
        return rc;
    return strip_merge<1, -1, -1>(what, s, g.part, strips, n, out_dev);
}

}  // extern "C"
