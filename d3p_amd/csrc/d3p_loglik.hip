// Pointwise log-likelihoods of the regression families over posterior draws (numpyro.infer.util.log_likelihood) and the log
// pointwise predictive density (d3p_amd/infer_util.py):
//   rows form   out[s, r] = ll[s, r] = log p(y_r | t[s, r]),  t[s, r] = X[r] . w_s (+ b_s)                     (n x rows)
//   lppd form   out[r]    = logsumexp_s ll[s, r] - log n                                                       (rows)
//   WAIC form   out[r]    = the lppd form's value, bit for bit;  pwaic[r] = Var_s ll[s, r] = M2 / (n - ddof)       (rows, rows)
// UNSCALED log-probabilities: no plate factor, no 1 / observation_scale (numpyro's log_likelihood returns fn.log_prob(value)).
//
// The product is the shared tile (d3p_glm_tile.h): 128 draws x 128 rows per workgroup, 4 wavefronts (2 x 2: wm = draw half, wn = row
// half) of 64 x 64.
//
// Epilogue, per half of a wave's 64 draws as in the predictive kernel: the accumulators go through LDS so that lane l owns row l
// and walks 32 draws; a rows-form store is 64 consecutive floats.  The lppd form's grid runs over row tiles only: a workgroup walks
// the draw tiles and every lane keeps a running (max, sum) of its row -- for each x = ll[s, r] in draw order
//   m' = max(m, x);  sum = sum exp(m - m') + exp(x - m')
// (one expf per element: whichever of the two exponents is 0 is not evaluated), the sum in float64 so that its roundings stay below
// float32 resolution for any n.  x = -inf adds nothing; while m = -inf the sum is 0, so a row whose every draw is -inf ends as -inf,
// never NaN; a NaN stays a NaN.  The two wm waves that share a row block are combined once at the end, wm = 0 then wm = 1, by the
// wm = 0 wave: deterministic, no atomics, no n x rows intermediate.
//
// The WAIC form (d3p_amd/criteria.py) is the lppd form with k_moments' shifted sums beside the running (max,
// sum), applied to x = ll[s, r] (d3p_shifted_sums.h): c = the wave's first finite x of the row, float64 sums of (x - c) and (x - c)^2,
// a count and flags.  The wm = 0 wave merges the two waves' parts in Chan's pairwise form, its own first (a wave with count 0 --
// n <= 64 leaves wm = 1 without a draw -- is left out, never divided by), and finishes pwaic = M2 / (n - ddof) in float64, rounded
// to float32 once.  Every draw of a row equal: pwaic is exactly 0.  Special values: x = -inf (Poisson rate overflow) is not added to
// the sums but remembered, and a row with at least one such draw gets pwaic = +inf -- also when every draw is -inf, where lppd = -inf.
// A NaN x makes both outputs of the row NaN.  x = +inf does not occur in these families for finite inputs; it is not added either,
// and makes pwaic NaN (lppd is then what the lppd form gives: +inf for one such draw, NaN from the second on).
#include "d3p_device.h"
#include "d3p_glm_tile.h"
#include "d3p_host.h"
#include "d3p_shifted_sums.h"

namespace d3p {

struct LoglikArgs {
    const float* X;
    const float* y;
    uint64_t rows;
    int d, w_off, b_col;
    const float* lat;
    int64_t ld;
    uint32_t n;
    float nh, ll_const;   // LINREG: -0.5 / sigma^2 and log sigma + log(2 pi) / 2, as the training kernels get them (d3p_dpvi.hip)
    float* out;
    float* pwaic;    // WAIC form
    uint32_t ddof;   // WAIC form: 0 or 1
};

// (loglik_value<FAMILY>, log p(y | t), is in d3p_glm_tile.h: the draw-sums form of d3p_draw_sums.hip evaluates the same text)

#define D3P_LOGLIK_ROWS 0
#define D3P_LOGLIK_LPPD 1
#define D3P_LOGLIK_WAIC 2

template <int FAMILY, int FORM>
// Registers: the rows form fits two waves per SIMD like k_predict_logreg; in the lppd form the compiler keeps the X addresses of the
// staging loads across the draw-tile loop, which at two waves per SIMD spills, so that form runs one wave per SIMD (no scratch), and
// the WAIC form with it.
__global__ void __launch_bounds__(256, FORM != D3P_LOGLIK_ROWS ? 1 : 2) k_loglik(LoglikArgs g)
{
    constexpr bool LPPD = FORM != D3P_LOGLIK_ROWS, WAIC = FORM == D3P_LOGLIK_WAIC;
    // [k][draw] | [k][row] during the product; afterwards the same bytes hold each wave's t, half a tile at a time (4 x 32 x 65 floats)
    __shared__ __attribute__((aligned(16))) float smem[D3P_TILE_SMEM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const uint64_t r0 = (uint64_t)blockIdx.x * D3P_TILE_N;
    // lane l owns row r in the epilogue: its label and the label's constant, once per row
    const uint64_t r = r0 + wn * 64 + lane;
    const bool live = r < g.rows;
    const float y = live ? g.y[r] : 0.f;
    const float c = FAMILY == D3P_FAMILY_POISSON ? lgammaf(y + 1.0f) : g.ll_const;
    float run_m = -INFINITY;
    double run_s = 0.0;
    double v1 = 0.0, v2 = 0.0;        // WAIC form: sum (x - vc), sum (x - vc)^2
    float vc = 0.f;                   //            the shift: this wave's first finite x of the row
    uint32_t vcnt = 0, vflags = 0;    //            values in the sums; D3P_SHIFTED_* flags
    uint32_t s0 = LPPD ? 0u : blockIdx.y * D3P_TILE_M;   // rows form: the grid's y runs over the draw tiles; lppd form: the loop does
    do {
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
                    const float x = loglik_value<FAMILY>(t, y, g.nh, c);
                    if (WAIC) shifted_add(x, vc, v1, v2, vcnt, vflags);
                    if (!LPPD) {
                        g.out[(size_t)s * g.rows + r] = x;
                    } else if (x > run_m) {          // new maximum: exp(x - m') = 1
                        run_s = run_s * (double)expf(run_m - x) + 1.0;
                        run_m = x;
                    } else if (x != -INFINITY) {     // exp(m - m') = 1; (x = m = -inf would be exp(nan)); a NaN x makes the sum NaN
                        run_s += (double)expf(x - run_m);
                    }
                }
            }
            __syncthreads();
        }
        s0 += D3P_TILE_M;
    } while (LPPD && s0 < g.n);
    if (LPPD) {
        // the two waves of a row block: wm = 1 hands its (max, sum) over, wm = 0 merges (its own first) and finishes in float64
        double* Ss = reinterpret_cast<double*>(smem);   // [128] sums, then [128] maxima behind them
        float* Ms = smem + 2 * D3P_TILE_N;
        // WAIC form, behind them: [2][128] shifted sums, then [128] shifts, counts and flags
        double* Vs = reinterpret_cast<double*>(smem + 3 * D3P_TILE_N);
        float* Cs = smem + 7 * D3P_TILE_N;
        uint32_t* Ks = reinterpret_cast<uint32_t*>(smem + 8 * D3P_TILE_N);
        uint32_t* Fs = reinterpret_cast<uint32_t*>(smem + 9 * D3P_TILE_N);
        const int slot = wn * 64 + lane;
        if (wm == 1) { Ss[wn * 64 + lane] = run_s; Ms[wn * 64 + lane] = run_m; }
        if (WAIC && wm == 1) { Vs[slot] = v1; Vs[D3P_TILE_N + slot] = v2; Cs[slot] = vc; Ks[slot] = vcnt; Fs[slot] = vflags; }
        __syncthreads();
        if (wm == 0 && live) {
            const double s1 = Ss[wn * 64 + lane];
            const float m1 = Ms[wn * 64 + lane];
            const float m = fmaxf(run_m, m1);
            // a wave that saw no finite value has sum 0 -- or NaN, if a NaN came by: it is taken as it is, so a NaN stays
            const double a0 = run_m == -INFINITY ? run_s : run_s * exp((double)run_m - (double)m);
            const double a1 = m1 == -INFINITY ? s1 : s1 * exp((double)m1 - (double)m);
            const double tot = a0 + a1;
            g.out[r] = (m == -INFINITY && tot == 0.0) ? -INFINITY : (float)(((double)m + log(tot)) - log((double)g.n));
            if (WAIC) {
                uint32_t ka = vcnt;
                const uint32_t kb = Ks[slot];
                double ma = 0.0, qa = 0.0, mb = 0.0, qb = 0.0;
                if (ka) moments_part(ka, vc, v1, v2, ma, qa);
                if (kb) moments_part(kb, Cs[slot], Vs[slot], Vs[D3P_TILE_N + slot], mb, qb);
                chan_merge(ka, ma, qa, kb, mb, qb);   // (neither: M2 = 0 -- every x was infinite, which the flags say)
                g.pwaic[r] = pwaic_value(qa, g.n, g.ddof, vflags | Fs[slot]);
            }
        }
    }
}

template <int FORM>
static int loglik_entry(const char* what, void* stream, const d3p_logreg_model* m, const float* X, const float* y, uint64_t rows, const float* latent,
                        int64_t ld, int32_t w_off, int32_t b_col, uint32_t n, float* out, float* pwaic = nullptr, uint32_t ddof = 0)
{
    constexpr bool WAIC = FORM == D3P_LOGLIK_WAIC;
    if (int rc = validate_model(m, y, what)) return rc;   // D3P_GUIDE_EXP_SITES: D3P_E_UNSUPPORTED (no form reads the guide transform otherwise)
    bool launch;
    if (int rc = WAIC ? glm_tile_check(what, m, rows, ld, w_off, b_col, n, {X, y, latent, out, pwaic}, "X / y / latent / lppd / pwaic",
                                       "X, y, latent, lppd and pwaic", &launch)
                      : glm_tile_check(what, m, rows, ld, w_off, b_col, n, {X, y, latent, out}, "X / y / latent / out", "X, y, latent and out", &launch);
        rc)
        return rc;
    if (WAIC && ddof > 1) return fail(D3P_E_INVALID_ARG, "%s: ddof must be 0 or 1 (got %u)", what, ddof);
    if (WAIC && n <= ddof) return fail(D3P_E_INVALID_ARG, "%s: n > ddof is required (n = %u, ddof = %u)", what, n, ddof);
    if (!launch) return D3P_OK;
    LoglikArgs g;
    g.X = X; g.y = y; g.rows = rows; g.d = m->d; g.w_off = w_off; g.b_col = b_col; g.lat = latent; g.ld = ld; g.n = n; g.out = out;
    g.pwaic = pwaic; g.ddof = ddof;
    // as the training kernels' arguments (d3p_dpvi.hip: nh_inv_var, ll_const)
    const bool sigma = m->family == D3P_FAMILY_LINREG;
    g.nh = sigma ? -0.5f / (m->lik_sigma * m->lik_sigma) : 0.f;
    g.ll_const = sigma ? logf(m->lik_sigma) + 0.91893853320467267f : 0.f;
    const dim3 grid(cdiv(rows, D3P_TILE_N), FORM != D3P_LOGLIK_ROWS ? 1u : cdiv(n, D3P_TILE_M));
    hipStream_t s = (hipStream_t)stream;
    if (m->family == D3P_FAMILY_LINREG) hipLaunchKernelGGL((k_loglik<D3P_FAMILY_LINREG, FORM>), grid, dim3(256), 0, s, g);
    else if (m->family == D3P_FAMILY_POISSON) hipLaunchKernelGGL((k_loglik<D3P_FAMILY_POISSON, FORM>), grid, dim3(256), 0, s, g);
    else hipLaunchKernelGGL((k_loglik<D3P_FAMILY_LOGREG, FORM>), grid, dim3(256), 0, s, g);
    return check_launch(what);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

int d3p_loglik_rows(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows, const float* latent_dev,
                    int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, float* out_dev)
{
    return loglik_entry<D3P_LOGLIK_ROWS>("d3p_loglik_rows", stream, model, X_dev, y_dev, rows, latent_dev, latent_ld, w_off, b_col, n, out_dev);
}

int d3p_loglik_lppd(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows, const float* latent_dev,
                    int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, float* out_rows_dev)
{
    return loglik_entry<D3P_LOGLIK_LPPD>("d3p_loglik_lppd", stream, model, X_dev, y_dev, rows, latent_dev, latent_ld, w_off, b_col, n, out_rows_dev);
}

int d3p_loglik_waic(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows, const float* latent_dev,
                    int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, uint32_t ddof, float* lppd_rows_dev, float* pwaic_rows_dev)
{
    return loglik_entry<D3P_LOGLIK_WAIC>("d3p_loglik_waic", stream, model, X_dev, y_dev, rows, latent_dev, latent_ld, w_off, b_col, n, lppd_rows_dev,
                                         pwaic_rows_dev, ddof);
}

}  // extern "C"
