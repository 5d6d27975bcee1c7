// The energy score of multivariate predictive draws against the observed outcomes (d3p_amd/energy.py, include/d3p_hip.h):
// the entry d3p_energy_score with its host checks, its kernels, the query functions of their tile constants and forms, and the test
// aid that forces a form.
//
// THE RULE.  draws[s * ld_draw + r * ld_row + c] is draw s < n of row r < rows in column c < d, float32 (dtype 0) or int32 (dtype 1:
// converted to float32 when staged, exact for |v| <= 2^24, which is what the Python layer admits); y[r * y_ld + c] the observation.
// For row r the ITEMS are z_0 .. z_{n-1} (the draws) and z_n = y_r.  For a pair of items (a, b):
//     t_c = fl32(a_c - b_c)      q = the float32 fmaf chain q <- fmaf(t_c, t_c, q) over c = 0 .. d-1 ascending, from q = 0
//     dist = the NATIVE root of q (1 ulp, exact on perfect squares; the bound of tests/energy_ref.bound carries it; DESIGN.md 4w's
//            kernel takes the IEEE root), widened to float64
// (the chain is symmetric in a and b: t_c only changes its sign).  With U = sum_{i<j<n} dist(z_i, z_j) in float64:
//     S1 = sum_{i<n} dist(z_i, y)      S2 = 2 U        (each unordered pair is computed once and counted twice)
//     mae = S1 / n      spread = S2 / (2 n^2)      es = mae - spread      es_fair = mae - S2 / (2 n (n - 1))   (n = 1: 0 / 0 = NaN is the rule)
// out[0 .. 3][r] = es, es_fair, mae, spread, each rounded to float32 once.  A NaN or +-inf element among a row's draws or in its y makes
// that row's four outputs NaN and touches no other row.  Finite elements whose t_c or q overflows float32 follow IEEE from there: dist =
// inf, so mae (and spread, if two draws are that far apart) is inf and es = inf - inf = NaN.
//
// THE ORDER of the float64 sums, which is one order for both forms (so the forms agree bit for bit):
//   * the items are cut into tiles of T = 32; the pair tiles (I, J), I <= J < ceil((n + 1) / T), are numbered t = 0, 1, .. row by row
//     (J ascending within I); tile t belongs to SLOT t mod 4;
//   * one wavefront computes a pair tile: lane l = 8 ti + tj owns the 4 x 4 pairs (i, j) = (32 I + ti + 8 ki, 32 J + tj + 8 kj) and adds
//     their dist in the order ki = 0 .. 3, kj = 0 .. 3 (kj fastest) onto its two float64 sums (towards S1 where j = n, towards U where
//     j < n; a pair with i >= j or j > n adds +0.0, which changes no bit of a non-negative sum), over the slot's tiles in ascending t;
//   * the 64 lanes of a slot are summed by the xor butterfly 32, 16, .. 1 (a + b is commutative: every lane ends with the same bits), and
//     the four slots are added in ascending order onto 0.
// The rows form (1) gives one wavefront a whole row: it walks the four slots one after the other; a workgroup of 4 wavefronts owns
// R = 16 adjacent rows (at step k its wavefronts hold rows 4 k .. 4 k + 3), so that at d = 2 the workgroup uses every byte of the 128-byte
// lines it fetches.  The streamed form (2) gives a workgroup one row and wavefront w slot w.  Either form walks the tile of
// d3p_pair_tile.h: the two sides of a pair tile staged in chunks of C = 32 columns in its wavefront's own LDS (2 x 32 x 36 floats; the
// row stride 36 keeps the 16-byte reads of the 8 distinct rows of a quarter wave on distinct banks), so neither n nor d is bounded by
// LDS; the pair accumulators q stay in registers across the
// chunks, which keeps the chain's order.  A chunk is padded with zeros to a multiple of 4 columns: fmaf(0, 0, q) = q for every q >= 0,
// NaN or inf.  Static LDS: 36944 bytes at most.  No floating-point atomics, no workspace, no host synchronisation, no dynamic LDS.
//
// DETERMINISM.  Repeated calls give equal bits.  A row's bits depend on that row's values, y, n and d alone: not on rows, the other rows,
// ld_draw, ld_row, y_ld, out_ld, the row's position within a workgroup, or the form.
//
// Distances are NOT taken from a Gram matrix (|a|^2 + |b|^2 - 2 a.b): for draws that sit close together far from the origin the
// cancellation loses every digit of the distance (out of scope).
#include "d3p_device.h"
#include "d3p_host.h"
#include "d3p_pair_tile.h"

#define D3P_ES_ROWS 16       // rows per workgroup of the rows form
#define D3P_ES_MAX_N 65535u
#define D3P_ES_FORM_ROWS 1
#define D3P_ES_FORM_STREAM 2
#define D3P_ES_ROWS_FORM_MIN_GROUPS 512u   // the rows form is chosen where it still fills the chip: rows >= 16 x 512

static int32_t g_es_form = 0;   // d3p_energy_score_set_form: 0 = the rule below

namespace d3p {

struct EsArgs {
    const uint32_t* z; const uint32_t* y; int32_t dtype; int64_t ld_draw, ld_row, y_ld; uint32_t n; uint64_t rows; uint32_t d;
    float* out; int64_t out_ld;
};

__device__ __forceinline__ double es_wave_sum(double v)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the items of row `row`: the n draws, then y as item n
struct EsItems {
    typedef uint32_t index;
    const uint32_t* z; const uint32_t* yrow; int64_t ld_draw; uint32_t n;
    __device__ __forceinline__ bool live(uint32_t item) const { return item <= n; }
    __device__ __forceinline__ uint32_t word(uint32_t item, uint32_t col) const { return (item < n ? z + (int64_t)item * ld_draw : yrow)[col]; }
};

// the tiles of one slot of one row: adds onto the lane's s1 (pairs with y) and u (pairs of draws), ors `bad`
__device__ __forceinline__ void es_row_slot(const EsArgs& a, uint64_t row, uint32_t slot, float* A, float* Bbuf, int lane, double& s1, double& u,
                                            bool& bad)
{
    const EsItems items = {a.z + (int64_t)row * a.ld_row, a.y + (int64_t)row * a.y_ld, a.ld_draw, a.n};
    const uint32_t nt = (a.n + 1u + D3P_PAIR_T - 1u) / D3P_PAIR_T;
    const uint32_t ti = (uint32_t)lane >> 3, tj = (uint32_t)lane & 7u;
    uint32_t t = 0;
    for (uint32_t I = 0; I < nt; ++I) {
        for (uint32_t J = I; J < nt; ++J, ++t) {
            if ((t & (D3P_PAIR_WAVES - 1u)) != slot) continue;
            const float* B = I == J ? A : Bbuf;
            float q[4][4];
            pair_zero(q);
            for (uint32_t c0 = 0; c0 < a.d; c0 += D3P_PAIR_C) {
                const uint32_t cw = a.d - c0 < D3P_PAIR_C ? a.d - c0 : D3P_PAIR_C;
                const int lw = pair_lanes_log2(cw);
                {
                    uint32_t wa[16], wb[16];
                    pair_load(items, I, c0, cw, lw, lane, wa);
                    if (I != J) pair_load(items, J, c0, cw, lw, lane, wb);
                    pair_wave_sync();   // the reads of the chunk before are done
                    pair_store(a.dtype, A, nullptr, lw, lane, wa, bad);
                    if (I != J) pair_store(a.dtype, Bbuf, nullptr, lw, lane, wb, bad);
                    pair_wave_sync();
                }
                const uint32_t cw4 = (cw + 3u) & ~3u;   // <= 2^lw: every column read below was written above
                for (uint32_t c = 0; c < cw4; c += 4) {
                    float4 va[4], vb[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        va[k] = *reinterpret_cast<const float4*>(A + (ti + 8u * k) * D3P_PAIR_LD + c);
                        vb[k] = *reinterpret_cast<const float4*>(B + (tj + 8u * k) * D3P_PAIR_LD + c);
                    }
#pragma unroll
                    for (int ki = 0; ki < 4; ++ki)
#pragma unroll
                        for (int kj = 0; kj < 4; ++kj) q[ki][kj] = pair_chain(va[ki], vb[kj], q[ki][kj]);
                }
            }
#pragma unroll
            for (int ki = 0; ki < 4; ++ki)
#pragma unroll
                for (int kj = 0; kj < 4; ++kj) {
                    const uint32_t i = I * D3P_PAIR_T + ti + 8u * ki, j = J * D3P_PAIR_T + tj + 8u * kj;
                    const double dist = (double)__fsqrt_rn(q[ki][kj]);
                    const bool pair = i < j && j <= a.n;
                    s1 += pair && j == a.n ? dist : 0.0;
                    u += pair && j < a.n ? dist : 0.0;
                }
        }
    }
}

__device__ __forceinline__ void es_finish(const EsArgs& a, uint64_t row, double s1, double u, bool bad)
{
    const double n = (double)a.n, s2 = 2.0 * u;
    const double mae = s1 / n, spread = s2 / (2.0 * n * n), fair = s2 / (2.0 * n * (n - 1.0));
    const float nan = __builtin_nanf("");
    a.out[0 * a.out_ld + (int64_t)row] = bad ? nan : (float)(mae - spread);
    a.out[1 * a.out_ld + (int64_t)row] = bad ? nan : (float)(mae - fair);
    a.out[2 * a.out_ld + (int64_t)row] = bad ? nan : (float)mae;
    a.out[3 * a.out_ld + (int64_t)row] = bad ? nan : (float)spread;
}

template <int FORM>
__global__ __launch_bounds__(64 * D3P_PAIR_WAVES) void k_energy_score(EsArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[D3P_PAIR_WAVES][2][D3P_PAIR_T * D3P_PAIR_LD];
    __shared__ double red[D3P_PAIR_WAVES][2];
    __shared__ uint32_t red_bad[D3P_PAIR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* A = lds[wave][0];
    float* B = lds[wave][1];
    if (FORM == D3P_ES_FORM_ROWS) {
        for (uint32_t k = 0; k < D3P_ES_ROWS / D3P_PAIR_WAVES; ++k) {
            const uint64_t row = (uint64_t)blockIdx.x * D3P_ES_ROWS + k * D3P_PAIR_WAVES + (uint32_t)wave;
            if (row >= a.rows) break;   // (wave-uniform; nothing below synchronises the workgroup)
            double S1 = 0.0, U = 0.0;
            bool bad = false;
            for (uint32_t slot = 0; slot < D3P_PAIR_WAVES; ++slot) {
                double s1 = 0.0, u = 0.0;
                es_row_slot(a, row, slot, A, B, lane, s1, u, bad);
                S1 += es_wave_sum(s1);
                U += es_wave_sum(u);
            }
            bad = __builtin_amdgcn_ballot_w64(bad) != 0ull;
            if (lane == 0) es_finish(a, row, S1, U, bad);
        }
    } else {
        const uint64_t row = blockIdx.x;
        double s1 = 0.0, u = 0.0;
        bool bad = false;
        es_row_slot(a, row, (uint32_t)wave, A, B, lane, s1, u, bad);
        s1 = es_wave_sum(s1);
        u = es_wave_sum(u);
        bad = __builtin_amdgcn_ballot_w64(bad) != 0ull;
        if (lane == 0) { red[wave][0] = s1; red[wave][1] = u; red_bad[wave] = bad ? 1u : 0u; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double S1 = 0.0, U = 0.0;
            uint32_t any = 0u;
            for (int w = 0; w < D3P_PAIR_WAVES; ++w) { S1 += red[w][0]; U += red[w][1]; any |= red_bad[w]; }
            es_finish(a, row, S1, U, any != 0u);
        }
    }
}

static uint32_t es_form(uint32_t n, uint64_t rows, uint32_t d)
{
    if (n < 1 || n > D3P_ES_MAX_N || d < 1) return 0;
    if (g_es_form) return (uint32_t)g_es_form;
    // an item shorter than a 128-byte line, and enough rows that workgroups of 16 rows still fill the chip; the forms agree bit for
    // bit, so the choice may look at rows
    return d < 32 && rows >= (uint64_t)D3P_ES_ROWS * D3P_ES_ROWS_FORM_MIN_GROUPS ? D3P_ES_FORM_ROWS : D3P_ES_FORM_STREAM;
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_energy_score_max_n(void) { return D3P_ES_MAX_N; }

uint32_t d3p_energy_score_tile_draws(void) { return D3P_PAIR_T; }

uint32_t d3p_energy_score_chunk_cols(void) { return D3P_PAIR_C; }

uint32_t d3p_energy_score_rows_per_group(int32_t form)
{
    return form == D3P_ES_FORM_ROWS ? D3P_ES_ROWS : form == D3P_ES_FORM_STREAM ? 1u : 0u;
}

uint32_t d3p_energy_score_form(uint32_t n, uint64_t rows, uint32_t d) { return es_form(n, rows, d); }

int d3p_energy_score_set_form(int32_t form)
{
    if (form != 0 && form != D3P_ES_FORM_ROWS && form != D3P_ES_FORM_STREAM)
        return fail(D3P_E_INVALID_ARG, "d3p_energy_score_set_form: form must be 0 (the rule), 1 (rows) or 2 (streamed), got %d", form);
    g_es_form = form;
    return D3P_OK;
}

int d3p_energy_score(void* stream, const void* draws_dev, int32_t dtype, int64_t ld_draw, int64_t ld_row, uint32_t n, uint64_t rows, uint32_t d,
                     const void* y_dev, int64_t y_ld, float* out_dev, int64_t out_ld)
{
    const char* what = "d3p_energy_score";
    if (!draws_dev || !y_dev || !out_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)draws_dev | (uintptr_t)y_dev | (uintptr_t)out_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: n >= 1 is required", what);
    if (d < 1) return fail(D3P_E_INVALID_ARG, "%s: d >= 1 is required", what);
    if (ld_row < 0 || (uint64_t)ld_row < d) return fail(D3P_E_INVALID_ARG, "%s: ld_row >= d is required", what);
    if (ld_draw < 0 || (uint64_t)ld_draw / (uint64_t)ld_row < rows)   // (ld_row >= d >= 1; no product that could wrap)
        return fail(D3P_E_INVALID_ARG, "%s: ld_draw >= rows * ld_row is required", what);
    if (y_ld < 0 || (uint64_t)y_ld < d) return fail(D3P_E_INVALID_ARG, "%s: y_ld >= d is required", what);
    if (out_ld < 0 || (uint64_t)out_ld < rows) return fail(D3P_E_INVALID_ARG, "%s: out_ld >= rows is required", what);
    if (n > D3P_ES_MAX_N)
        return fail(D3P_E_UNSUPPORTED, "%s: n = %u draws; n <= %u is served (one workgroup walks all pairs of a row)", what, n, D3P_ES_MAX_N);
    if (ld_draw != 0 && (uint64_t)(n - 1u) > (uint64_t)INT64_MAX / (uint64_t)ld_draw)
        return fail(D3P_E_INVALID_ARG, "%s: n * ld_draw does not fit 63 bits", what);
    const uint32_t form = es_form(n, rows, d);
    const uint64_t per = d3p_energy_score_rows_per_group((int32_t)form);
    const uint64_t groups = rows / per + (rows % per ? 1u : 0u);
    if (groups > 0x7fffffffull) return fail(D3P_E_UNSUPPORTED, "%s: more than 2^31 - 1 workgroups (%u rows each)", what, (unsigned)per);
    if (rows == 0) return D3P_OK;
    if (!is_device_ptr(draws_dev) || !is_device_ptr(y_dev) || !is_device_ptr(out_dev))
        return fail(D3P_E_INVALID_ARG, "%s: the draws, the observations and the output must be device memory", what);
    EsArgs a;
    a.z = static_cast<const uint32_t*>(draws_dev); a.y = static_cast<const uint32_t*>(y_dev); a.dtype = dtype; a.ld_draw = ld_draw;
    a.ld_row = ld_row; a.y_ld = y_ld; a.n = n; a.rows = rows; a.d = d; a.out = out_dev; a.out_ld = out_ld;
    if (form == D3P_ES_FORM_ROWS)
        hipLaunchKernelGGL(k_energy_score<D3P_ES_FORM_ROWS>, dim3((unsigned)groups), dim3(64 * D3P_PAIR_WAVES), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_energy_score<D3P_ES_FORM_STREAM>, dim3((unsigned)groups), dim3(64 * D3P_PAIR_WAVES), 0, (hipStream_t)stream, a);
    return check_launch(what);
}

}  // extern "C"
