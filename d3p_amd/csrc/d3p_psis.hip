// PSIS-LOO (Pareto-smoothed importance-sampling leave-one-out; Vehtari, Gelman & Gabry 2017, Vehtari et al. 2024) per row of a
// draws x rows float32 log-likelihood matrix: d3p_psis_loo (include/d3p_hip.h, d3p_amd/criteria.py).  The kernel knows
// nothing of the model: the matrix is what d3p_loglik_rows / d3p_gmm_loglik_rows write.
//
// One workgroup of 256 threads owns D3P_PS_ROWS = 32 adjacent rows (one 128-byte line of every draw's row of the matrix).
//   scan phase   thread t = (draw lane t / 32, row lane t % 32): the 8 draw lanes of a row take the draws dl, dl + 8, ... in every pass
//                over the column; a wave reads two whole lines per load.  Per-row partials meet in LDS and are combined in the order
//                dl = 0 .. 7.  Passes: (1) min, max and the NaN / +inf / -inf flags; (2) the lppd sum and the first of four 8-bit
//                radix-select passes over the order-preserving uint32 image of ll (integer LDS atomics on a 32 x 256 histogram);
//                (3-5) the other three; (6) the tail (x > cut) gathered into LDS, the rest summed.  x[s] = min_s ll - ll[s] is
//                decreasing in ll, so the (M+1)-th largest x is the image of the (M+1)-th smallest ll: the selection is exact on
//                the float32 values, and membership is decided by the float64 comparison x > cut the definition states.
//   fit phase    wave w takes the rows w, w + 4, ...: the tail (T <= M <= 768 float32 values) is sorted by counting ranks (ties get
//                consecutive ranks; equal values are interchangeable in every sum below, so no draw index is kept), e_j goes to a
//                float64 buffer of the wave, lane i < m = 30 + floor(sqrt T) runs candidate b_i over the tail sequentially (LDS
//                broadcast reads, no cross-lane traffic in the m T log1p calls that dominate), the weights and b are sums over the
//                lanes in the order 0 .. m - 1, and the sums over the tail that follow (k, the smoothed numerator and denominator)
//                are 64 strided partials (lane l: j = l, l + 64, ...) merged by an xor butterfly 32, 16, .., 1.
// All arithmetic after the loads is float64, the three outputs are rounded once.  Nothing is atomic in floating point, every order
// above is fixed and a row meets no other row's values: identical bits between calls and for any set of other rows in the launch.
#include "d3p_colreduce.h"

#include <float.h>

#pragma clang fp contract(off)

namespace d3p {

#define D3P_PS_ROWS 32
#define D3P_PS_DL 8
#define D3P_PS_WAVES 4
#define D3P_PS_HSTRIDE 257            // 256 bins + 1: the 32 row lanes of a histogram update fall on 32 banks
#define D3P_PS_LOG_DBL_MIN (-708.3964185322641)   // log(DBL_MIN), as correctly rounded

struct PsisArgs {
    const float* ll;
    int64_t ld;
    uint64_t rows;
    uint32_t n, M, rank;   // rank = min(M + 1, n): the cut is the rank-th smallest ll (1-based)
    float *elpd, *lppd, *k;
};

__host__ __device__ inline size_t ps_region_bytes(uint32_t M)
{
    const size_t hist = (size_t)D3P_PS_ROWS * D3P_PS_HSTRIDE * 4, tail = (size_t)D3P_PS_ROWS * M * 4;
    return hist > tail ? hist : tail;
}

// [E: 4 waves x M float64][histogram, later the 32 rows' tails: 32 x M float32][S: 4 waves x M float32]
inline size_t ps_lds_bytes(uint32_t M) { return (size_t)D3P_PS_WAVES * M * 8 + ps_region_bytes(M) + (size_t)D3P_PS_WAVES * M * 4; }

__device__ inline double ps_wave_sum(double v)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ inline double ps_wave_max(double v)
{
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(256) void k_psis_loo(PsisArgs a)
{
    extern __shared__ __align__(16) unsigned char ps_smem[];
    const uint32_t M = a.M, n = a.n;
    double* E = reinterpret_cast<double*>(ps_smem);
    unsigned char* region = ps_smem + (size_t)D3P_PS_WAVES * M * 8;
    uint32_t* hist = reinterpret_cast<uint32_t*>(region);
    float* tail = reinterpret_cast<float*>(region);
    float* S = reinterpret_cast<float*>(region + ps_region_bytes(M));

    __shared__ double r_d0[D3P_PS_DL][D3P_PS_ROWS], r_d1[D3P_PS_DL][D3P_PS_ROWS];
    __shared__ float r_f0[D3P_PS_DL][D3P_PS_ROWS], r_f1[D3P_PS_DL][D3P_PS_ROWS];
    __shared__ uint32_t r_u[D3P_PS_DL][D3P_PS_ROWS];
    __shared__ double s_lppd[D3P_PS_ROWS], s_cut[D3P_PS_ROWS], s_dnt[D3P_PS_ROWS], s_nnt[D3P_PS_ROWS];
    __shared__ float s_min[D3P_PS_ROWS], s_max[D3P_PS_ROWS];
    __shared__ uint32_t s_flags[D3P_PS_ROWS], s_prefix[D3P_PS_ROWS], s_rank[D3P_PS_ROWS], s_cnt[D3P_PS_ROWS];

    const int t = threadIdx.x, rl = t & (D3P_PS_ROWS - 1), dl = t >> 5;
    const uint64_t r = (uint64_t)blockIdx.x * D3P_PS_ROWS + rl;
    const bool live = r < a.rows;                       // a row past the end stands for n draws of 0 and writes nothing
    const float* col = a.ll + (live ? r : 0);
    const size_t ld = (size_t)a.ld;
#define PS_LOAD(s) (live ? col[(size_t)(s) * ld] : 0.0f)

    // pass 1: min, max, flags (1: a NaN, 2: a +inf, 4: a -inf)
    float mn = INFINITY, mx = -INFINITY;
    uint32_t fl = 0;
    for (uint32_t s = dl; s < n; s += D3P_PS_DL) {
        const float v = PS_LOAD(s);
        fl |= (v != v ? 1u : 0u) | (v == INFINITY ? 2u : 0u) | (v == -INFINITY ? 4u : 0u);
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    r_f0[dl][rl] = mn; r_f1[dl][rl] = mx; r_u[dl][rl] = fl;
    __syncthreads();
    for (int q = 0; q < D3P_PS_DL; ++q) { mn = fminf(mn, r_f0[q][rl]); mx = fmaxf(mx, r_f1[q][rl]); fl |= r_u[q][rl]; }
    const double mnd = (double)mn, mxd = (double)mx;

    // passes 2-5: the radix select of the rank-th smallest ll, most significant byte first; the lppd sum rides on the first
    for (int p = 0; p < 4; ++p) {
        for (int i = t; i < D3P_PS_ROWS * D3P_PS_HSTRIDE; i += 256) hist[i] = 0u;
        __syncthreads();
        const int shift = 24 - 8 * p;
        const uint32_t prefix = p ? s_prefix[rl] : 0u;
        double sum = 0.0;
        for (uint32_t s = dl; s < n; s += D3P_PS_DL) {
            const float v = PS_LOAD(s);
            const uint32_t key = key_f32(__float_as_uint(v));
            if (p == 0) {
                sum += exp((double)v - mxd);
                atomicAdd(&hist[rl * D3P_PS_HSTRIDE + (key >> 24)], 1u);
            } else if ((key >> (shift + 8)) == prefix) {
                atomicAdd(&hist[rl * D3P_PS_HSTRIDE + ((key >> shift) & 255u)], 1u);
            }
        }
        if (p == 0) r_d0[dl][rl] = sum;
        __syncthreads();
        if (dl == 0) {
            if (p == 0) {
                double tot = 0.0;
                for (int q = 0; q < D3P_PS_DL; ++q) tot += r_d0[q][rl];
                s_lppd[rl] = mxd + log(tot) - log((double)n);
            }
            uint32_t want = p ? s_rank[rl] : a.rank, cum = 0u, bin = 255u;
            for (uint32_t b = 0; b < 256u; ++b) {
                const uint32_t c = hist[rl * D3P_PS_HSTRIDE + b];
                if (cum + c >= want) { bin = b; break; }
                cum += c;
            }
            s_prefix[rl] = (prefix << 8) | bin;
            s_rank[rl] = want > cum ? want - cum : 1u;
            if (p == 3) s_cnt[rl] = 0u;
        }
        __syncthreads();
    }

    // pass 6: the tail into LDS (over the histogram), the rest into the two sums that need no smoothing
    const double cut = fmax(mnd - (double)f32_of_key(s_prefix[rl]), D3P_PS_LOG_DBL_MIN);
    {
        double dnt = 0.0, nnt = 0.0;
        for (uint32_t s = dl; s < n; s += D3P_PS_DL) {
            const float v = PS_LOAD(s);
            const double x = mnd - (double)v;
            if (x > cut) {
                const uint32_t pos = atomicAdd(&s_cnt[rl], 1u);
                if (pos < M) tail[(size_t)rl * M + pos] = v;
            } else {
                dnt += exp(x);
                nnt += exp((x + (double)v) - mnd);
            }
        }
        r_d0[dl][rl] = dnt; r_d1[dl][rl] = nnt;
    }
    __syncthreads();
    if (dl == 0) {
        double dnt = 0.0, nnt = 0.0;
        for (int q = 0; q < D3P_PS_DL; ++q) { dnt += r_d0[q][rl]; nnt += r_d1[q][rl]; }
        s_dnt[rl] = dnt; s_nnt[rl] = nnt; s_cut[rl] = cut; s_min[rl] = mn; s_max[rl] = mx; s_flags[rl] = fl;
    }
    __syncthreads();
#undef PS_LOAD

    // fit phase: one wave per row
    const int w = t >> 6, lane = t & 63;
    double* Ew = E + (size_t)w * M;
    float* Sw = S + (size_t)w * M;
    for (int it = 0; it < D3P_PS_ROWS / D3P_PS_WAVES; ++it) {
        const int row = it * D3P_PS_WAVES + w;
        const float* tl = tail + (size_t)row * M;
        const uint32_t T = s_cnt[row] < M ? s_cnt[row] : M;
        const uint32_t flags = s_flags[row];
        const double rmin = (double)s_min[row], rcut = s_cut[row];
        // ascending x = descending ll; equal values take consecutive ranks
        for (uint32_t j = lane; j < T; j += 64) {
            const float v = tl[j];
            uint32_t rank = 0;
            for (uint32_t i = 0; i < T; ++i) {
                const float u = tl[i];
                rank += (u > v || (u == v && i < j)) ? 1u : 0u;
            }
            Sw[rank] = v;
        }
        __syncthreads();
        const bool fit = T > 4u && flags == 0u;
        const double ecut = exp(rcut), Td = (double)T;
        if (fit)
            for (uint32_t j = lane; j < T; j += 64) Ew[j] = exp(rmin - (double)Sw[j]) - ecut;
        __syncthreads();
        bool ok = false;
        double kreg = 0.0, sigma = 0.0;
        if (fit) {
            const uint32_t m = 30u + (uint32_t)sqrt(Td), q = (uint32_t)(Td * 0.25 + 0.5);
            const double eT = Ew[T - 1], eq = Ew[q - 1];
            const uint32_t i = (uint32_t)lane < m ? (uint32_t)lane : m - 1;
            const double bi = 1.0 / eT + (1.0 - sqrt((double)m / ((double)i + 0.5))) / (3.0 * eq);
            double acc = 0.0;
            for (uint32_t j = 0; j < T; ++j) acc += log1p(-bi * Ew[j]);
            const double ki = acc / Td;
            const double Li = Td * (log(-bi / ki) - ki - 1.0);
            double den = 0.0;
            for (uint32_t j = 0; j < m; ++j) den += exp(__shfl(Li, (int)j) - Li);
            double wi = 1.0 / den;
            if ((uint32_t)lane >= m || wi < 10.0 * DBL_EPSILON) wi = 0.0;
            double sw = 0.0;
            for (uint32_t j = 0; j < m; ++j) sw += __shfl(wi, (int)j);
            const double wb = (wi / sw) * bi;
            double b = 0.0;
            for (uint32_t j = 0; j < m; ++j) b += __shfl(wb, (int)j);
            double part = 0.0;
            for (uint32_t j = lane; j < T; j += 64) part += log1p(-b * Ew[j]);
            const double k = ps_wave_sum(part) / Td;
            sigma = -k / b;
            kreg = (Td * k + 5.0) / (Td + 10.0);
            ok = isfinite(k) && isfinite(sigma) && sigma > 0.0;
        }
        __syncthreads();   // (every read of e_j is done: the buffer now takes x_j + ll_j)
        double dpart = 0.0, lmax = -INFINITY;
        for (uint32_t j = lane; j < T; j += 64) {
            const double sv = (double)Sw[j];
            double xn = rmin - sv;
            if (ok) {
                const double lp = log1p(-(((double)j + 0.5) / Td));
                const double qv = fabs(kreg) < DBL_EPSILON ? -sigma * lp : sigma * expm1(-kreg * lp) / kreg;
                xn = fmin(0.0, log(ecut + qv));
            }
            const double v = xn + sv;
            Ew[j] = v;
            dpart += exp(xn);
            lmax = fmax(lmax, v);
        }
        const double den = s_dnt[row] + ps_wave_sum(dpart);
        const double top = fmax(ps_wave_max(lmax), rmin);   // (n - T >= 1 draws stay outside the tail, each at x + ll = min ll)
        double npart = 0.0;
        for (uint32_t j = lane; j < T; j += 64) npart += exp(Ew[j] - top);
        const double num = s_nnt[row] * exp(rmin - top) + ps_wave_sum(npart);
        const uint64_t rg = (uint64_t)blockIdx.x * D3P_PS_ROWS + row;
        if (lane == 0 && rg < a.rows) {
            float elpd = (float)(top + log(num) - log(den)), kk = ok ? (float)kreg : INFINITY, lppd = (float)s_lppd[row];
            if (flags & 1u) {
                elpd = kk = lppd = NAN;
            } else if (flags & 2u) {
                elpd = kk = NAN;
                lppd = INFINITY;
            } else if (flags & 4u) {
                elpd = -INFINITY;
                kk = INFINITY;
                if (s_max[row] == -INFINITY) lppd = -INFINITY;
            }
            a.elpd[rg] = elpd;
            a.lppd[rg] = lppd;
            a.k[rg] = kk;
        }
        __syncthreads();
    }
}

}  // namespace d3p

using namespace d3p;

extern "C" int d3p_psis_loo(void* stream, const float* ll_dev, int64_t ll_ld, uint32_t n, uint64_t rows, float* elpd_rows_dev,
                            float* lppd_rows_dev, float* k_rows_dev)
{
    const char* what = "d3p_psis_loo";
    if (!ll_dev || !elpd_rows_dev || !lppd_rows_dev || !k_rows_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if (!aligned4(ll_dev) || !aligned4(elpd_rows_dev) || !aligned4(lppd_rows_dev) || !aligned4(k_rows_dev))
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (n < 1 || n > 65535u) return fail(D3P_E_INVALID_ARG, "%s: 1 <= n <= 65535 (n = %u)", what, n);
    if (ll_ld < 0 || (uint64_t)ll_ld < rows) return fail(D3P_E_INVALID_ARG, "%s: ll_ld >= rows is required", what);
    if (rows == 0) return D3P_OK;
    if (rows > (uint64_t)0x7fffffff * D3P_PS_ROWS) return fail(D3P_E_UNSUPPORTED, "%s: rows <= 32 (2^31 - 1)", what);
    if (!is_device_ptr(ll_dev) || !is_device_ptr(elpd_rows_dev) || !is_device_ptr(lppd_rows_dev) || !is_device_ptr(k_rows_dev))
        return fail(D3P_E_INVALID_ARG, "%s: every pointer must be device memory", what);
    PsisArgs a;
    a.ll = ll_dev; a.ld = ll_ld; a.rows = rows; a.n = n; a.elpd = elpd_rows_dev; a.lppd = lppd_rows_dev; a.k = k_rows_dev;
    const double dn = (double)n, by_sqrt = 3.0 * sqrt(dn);
    a.M = (uint32_t)ceil(dn / 5.0 < by_sqrt ? dn / 5.0 : by_sqrt);   // relative efficiency 1: M <= 768 at n <= 65535
    a.rank = a.M + 1 < n ? a.M + 1 : n;
    const size_t lds = ps_lds_bytes(a.M);
    if (lds > (size_t)D3P_DYN_LDS_MAX) return fail(D3P_E_UNSUPPORTED, "%s: %zu bytes of LDS needed (M = %u)", what, lds, a.M);
    if (lds > 48u * 1024u)
        if (int rc = dynamic_lds_opt_in(reinterpret_cast<const void*>(&k_psis_loo), D3P_DYN_LDS_MAX, what)) return rc;
    hipLaunchKernelGGL(k_psis_loo, dim3((unsigned)((rows + D3P_PS_ROWS - 1) / D3P_PS_ROWS)), dim3(256), lds, (hipStream_t)stream, a);
    return check_launch(what);
}
