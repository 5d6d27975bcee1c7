// Between-draw moments of a lane's values without cancellation, shared by k_moments (d3p_moments.hip) and the WAIC forms of k_loglik
// (d3p_loglik.hip) and k_gmm_density (d3p_gmm_density.hip): per wave and row the sums of (x - c) and (x - c)^2 in float64, c the
// wave's first finite x of the row, so that S2 - S1^2 / k loses nothing to the size of x and is exactly 0 when every x is equal; the
// waves' parts are merged in Chan's pairwise form in a fixed order.
#pragma once
#include "d3p_device.h"

namespace d3p {

// (count, mean, sum of squared deviations from it) of the k values whose sums shifted by c are s1, s2; k >= 1
__device__ __forceinline__ void moments_part(uint32_t k, float c, double s1, double s2, double& mean, double& m2)
{
    const double kd = (double)k;
    mean = (double)c + s1 / kd;
    const double r = s2 - (s1 * s1) / kd;
    m2 = r < 0.0 ? 0.0 : r;   // (a NaN stays)
}

#define D3P_SHIFTED_NEG_INF 1u   // flags: a -inf x came by
#define D3P_SHIFTED_POS_INF 2u   //        a +inf x came by

// One x in draw order.  An infinite x is not added (inf - inf) but remembered in flags; a NaN x is added and makes the sums NaN.
__device__ __forceinline__ void shifted_add(float x, float& c, double& s1, double& s2, uint32_t& cnt, uint32_t& flags)
{
    if (fabsf(x) == INFINITY) {
        flags |= x < 0.0f ? D3P_SHIFTED_NEG_INF : D3P_SHIFTED_POS_INF;
        return;
    }
    if (cnt == 0) c = x;
    const double dv = (double)x - (double)c;
    s1 += dv;
    s2 += dv * dv;
    ++cnt;
}

// Chan's pairwise merge of part b into part a (count, mean, M2).  A part with count 0 is left out and never divided by.
__device__ __forceinline__ void chan_merge(uint32_t& ka, double& ma, double& qa, uint32_t kb, double mb, double qb)
{
    if (!kb) return;
    if (!ka) { ka = kb; ma = mb; qa = qb; return; }
    const double tot = (double)ka + (double)kb, delta = mb - ma;
    ma = ma + delta * ((double)kb / tot);
    qa = (qa + qb) + (delta * delta) * ((double)ka * (double)kb / tot);
    ka += kb;
}

// p_waic of a row from its merged M2 over n draws: M2 / (n - ddof) in float64, rounded once.  A NaN stays; a +inf x makes it NaN
// (the variance of a set with +inf in it is inf - inf); otherwise a -inf x makes it +inf.
__device__ __forceinline__ float pwaic_value(double m2, uint32_t n, uint32_t ddof, uint32_t flags)
{
    double p = m2 / (double)(n - ddof);
    if (flags & D3P_SHIFTED_POS_INF) p = (double)NAN;
    else if ((flags & D3P_SHIFTED_NEG_INF) && !(p != p)) p = (double)INFINITY;
    return (float)p;
}

}  // namespace d3p
