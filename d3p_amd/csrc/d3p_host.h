// Host-side helpers of libd3p_hip.so: error reporting and launch checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <cmath>

#include "../../include/d3p_hip.h"

namespace d3p {

char* last_error_buf();  // thread-local, 512 bytes

inline int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

inline int check_launch(const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(D3P_E_HIP, "%s: %s", what, hipGetErrorString(e));
    return D3P_OK;
}

#define D3P_HIP_TRY(expr)                                                                   \
    do {                                                                                    \
        hipError_t e__ = (expr);                                                            \
        if (e__ != hipSuccess) return d3p::fail(D3P_E_HIP, "%s: %s", #expr, hipGetErrorString(e__)); \
    } while (0)

#define D3P_REQUIRE(cond, msg)                                         \
    do {                                                               \
        if (!(cond)) return d3p::fail(D3P_E_INVALID_ARG, "%s", msg);   \
    } while (0)

// the generalised linear models that share the logistic regression's kernels through glm_link (d3p_logreg_kernel.h)
inline bool is_glm(const d3p_logreg_model* m) { return m->family == D3P_FAMILY_LINREG || m->family == D3P_FAMILY_POISSON; }

// Those two families run on one GPU: an entry point of the data-parallel loops (a communicator, an exchange, or a row range that is
// not the whole table) refuses them before any launch.
inline int refuse_glm_shards(const d3p_logreg_model* m, const d3p_batch_source* src, bool data_parallel_entry, const char* what)
{
    if (m && is_glm(m) && (data_parallel_entry || (src && !(src->row_lo == 0 && src->row_hi == src->n_rows))))
        return fail(D3P_E_UNSUPPORTED, "%s: linear / Poisson regression run on one GPU (the whole table: row_lo = 0, row_hi = n_rows)", what);
    return D3P_OK;
}

// model spec checks shared by every entry point that takes a d3p_logreg_model; labels are read by
// every family but the Gaussian mean.  allow_sites: the entry point runs D3P_GUIDE_EXP_SITES (the single-GPU runs); every other one refuses it.
inline int validate_model(const d3p_logreg_model* m, const void* y_dev, const char* what, bool allow_sites = false)
{
    if (!m) return fail(D3P_E_INVALID_ARG, "%s: null model", what);
    if (!(m->d >= 1 && m->prior_w > 0.f && m->prior_b > 0.f && m->inv_obs > 0.f))
        return fail(D3P_E_INVALID_ARG, "%s: bad model (d >= 1, prior scales > 0 and inv_obs > 0 are required)", what);
    if (m->guide_transform == D3P_GUIDE_EXP_SITES) {
        if (!allow_sites)
            return fail(D3P_E_UNSUPPORTED, "%s: guide transform D3P_GUIDE_EXP_SITES (state in tree order) is run by the single-GPU "
                        "runs only", what);
        if (is_glm(m))
            return fail(D3P_E_UNSUPPORTED, "%s: D3P_GUIDE_EXP_SITES is built for logistic regression only (linear / Poisson regression: "
                        "D3P_GUIDE_SOFTPLUS or D3P_GUIDE_EXP)", what);
        if (!(m->intercept && m->family == D3P_FAMILY_LOGREG))
            return fail(D3P_E_INVALID_ARG, "%s: D3P_GUIDE_EXP_SITES needs logistic regression with an intercept", what);
    } else if (m->guide_transform != D3P_GUIDE_SOFTPLUS && m->guide_transform != D3P_GUIDE_EXP) {
        return fail(D3P_E_INVALID_ARG, "%s: unknown guide transform %d", what, m->guide_transform);
    }
    if (m->family == D3P_FAMILY_LOGREG) {
        if (!y_dev) return fail(D3P_E_INVALID_ARG, "%s: null label pointer", what);
    } else if (m->family == D3P_FAMILY_GAUSS_MEAN) {
        if (m->intercept) return fail(D3P_E_INVALID_ARG, "%s: the Gaussian-mean family has no intercept", what);
        if (!(m->lik_sigma > 0.f)) return fail(D3P_E_INVALID_ARG, "%s: lik_sigma must be > 0", what);
    } else if (is_glm(m)) {
        if (!y_dev) return fail(D3P_E_INVALID_ARG, "%s: null label pointer", what);
        if (m->family == D3P_FAMILY_LINREG && !(m->lik_sigma > 0.f && std::isfinite(m->lik_sigma)))
            return fail(D3P_E_INVALID_ARG, "%s: lik_sigma must be finite and > 0", what);
    } else {
        return fail(D3P_E_INVALID_ARG, "%s: unknown likelihood family %d", what, m->family);
    }
    return D3P_OK;
}

// device (or managed) memory of this process: a host pointer must never reach a kernel
inline bool is_device_ptr(const void* p)
{
    if (!p) return false;
    hipPointerAttribute_t at;
    const hipError_t e = hipPointerGetAttributes(&at, p);
    (void)hipGetLastError();   // an unregistered host pointer leaves an error behind; it must not be reported by a later launch check
    return e == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
}

#define D3P_REQUIRE_DEV(p, msg) D3P_REQUIRE(d3p::is_device_ptr(p), msg)

inline unsigned cdiv(unsigned long long a, unsigned long long b) { return (unsigned)((a + b - 1) / b); }

// in-place sum-all-reduce of `count` floats over the ranks of a d3p_comm_* communicator (RCCL, resolved at run time: d3p_dpvi.hip)
int rccl_allreduce_f32(void* comm, float* buf, size_t count, hipStream_t s);

// in-place sum-all-reduce of the n floats a d3p_fmesh_* mesh was created for (full-mesh reduce-scatter + all-gather over the peers'
// hipIpc-mapped inboxes: d3p_fmesh.hip)
int fmesh_enqueue_allreduce(hipStream_t s, void* fmesh, float* buf, uint64_t n);

}  // namespace d3p
