// What the model-free reducers over a draws x columns matrix share: d3p_psis.hip, d3p_quantiles.hip, d3p_hpdi.hip and
// d3p_grad_norms.hip select or sort on ONE order-preserving uint32 key and interpolate by ONE rule; they and the mixture's files
// (d3p_gmm_density.hip, d3p_predict_gmm.hip) share the host checks below.  A new column reducer includes this header and defines no
// key map of its own; one that needs the whole sorted column (k_col_hpdi, and k_col_crps of d3p_crps_kernel.h, both compiled in
// d3p_hpdi.hip) uses d3p_colsort.h behind this header and defines no sort, no key staging and no form rule of its own either.  The
// training translation units do not include it.
#pragma once
#include "d3p_host.h"

#include <mutex>
#include <utility>
#include <vector>

namespace d3p {

// ---- device: the order keys ------------------------------------------------------------------------------------------------------------
// Order-preserving uint32 image of a stored float32 word (-0 taken as +0: they are one value): a < b as floats <=> key(a) < key(b).
__device__ inline uint32_t key_f32(uint32_t u)
{
    if ((u << 1) == 0u) u = 0u;
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ inline uint32_t key_i32(uint32_t u) { return u ^ 0x80000000u; }   // of a stored int32 word: the sign bit flipped
__device__ inline uint32_t key_of(uint32_t u, int32_t dtype) { return dtype ? key_i32(u) : key_f32(u); }   // dtype 0: float32, 1: int32

// The stored value of a key.  What an int32 becomes (an exact double, a float32 rounded once) is the caller's cast.
__device__ inline float f32_of_key(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ inline int32_t i32_of_key(uint32_t k) { return (int32_t)(k ^ 0x80000000u); }

// a float32's raw word
__device__ inline bool word_is_nan(uint32_t u) { return (u << 1) > 0xff000000u; }
__device__ inline bool word_is_finite(uint32_t u) { return (u << 1) < 0xff000000u; }

// numpy's method='linear' between two selected values va <= vb, a fraction g of the way.  One infinite end: the other's side of the
// rule gives that end; (-inf, +inf): NaN.
__device__ inline double lerp_linear(double va, double vb, double g)
{
#pragma clang fp contract(off)   // (here, not at file scope: an includer's own setting is not this header's to change)
    if (g == 0.0 || va == vb) return va;
    if (fabs(va) == (double)INFINITY || fabs(vb) == (double)INFINITY)
        return fabs(va) != (double)INFINITY ? vb : fabs(vb) != (double)INFINITY ? va : (double)NAN;
    const double d = vb - va;
    return g < 0.5 ? va + d * g : vb - d * (1.0 - g);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// 144 KiB of dynamic LDS: what the key buffers of k_psis_loo, k_col_quantiles, k_col_hpdi and k_col_crps may take beside at most 9 KiB of static
// LDS within a compute unit's 160 KiB
#define D3P_DYN_LDS_MAX 147456

// More than 48 KiB of dynamic LDS needs an opt-in per function and device.  `bytes` is the kernel's fixed maximum, not a launch's
// figure: the attribute is set once.
inline int dynamic_lds_opt_in(const void* fn, int bytes, const char* what)
{
    static std::mutex mu;
    static std::vector<std::pair<const void*, int>> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    std::lock_guard<std::mutex> lock(mu);
    for (const auto& e : done)
        if (e.first == fn && e.second == dev) return D3P_OK;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        char figure[16] = "";   // (only a maximum of its own is named)
        if (bytes != D3P_DYN_LDS_MAX) snprintf(figure, sizeof(figure), ", %d", bytes);
        return fail(D3P_E_HIP, "%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize%s) on device %d: %s", what, figure, dev, hipGetErrorString(e));
    }
    done.emplace_back(fn, dev);
    return D3P_OK;
}

}  // namespace d3p
