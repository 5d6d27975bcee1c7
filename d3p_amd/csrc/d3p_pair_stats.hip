// Pair statistics of two tables (d3p_amd/fidelity.py, include/d3p_hip.h): per row of the first table the float64 sum of its
// distances to the rows of the second, the distance to its nearest row there and that row's index -- what the two-sample energy distance,
// the distance to the closest record and the nearest-neighbour adversarial accuracy of a synthetic table reduce.  The entry
// d3p_pair_stats with its host checks, its kernels, the query functions of their constants, forms and workspace, and the test aid that
// forces a form.
//
// THE RULE.  a[i * a_ld + c] is row i < na of the first table in column c < d, b[j * b_ld + c] row j < nb of the second, both float32
// (dtype 0) or both int32 (dtype 1: converted to float32 when staged, exact for |v| <= 2^24, which is what the Python layer admits).
// For a pair of rows (i, j):
//     t_c = fl32(a_c - b_c)      q = the float32 fmaf chain q <- fmaf(t_c, t_c, q) over c = 0 .. d-1 ascending, from q = 0
//     dist = sqrtf(q), correctly rounded (the IEEE root: ps_sqrt below, not the native instruction's 1 ulp)
// which is the chain of d3p_energy.hip: both walk the tile of d3p_pair_tile.h.  The ADMISSIBLE j of row i are all j < nb, without j == i when
// exclude_diagonal is set (which requires na == nb); duplicate rows are pairs like any other.  Over the admissible j:
//     sum[i]    = sum_j (double)dist(i, j)     in float64, in the order below, not rounded further
//     min[i]    = sqrtf(q_min),  q_min the smallest q
//     argmin[i] = the SMALLEST j whose q equals q_min   (the tie rule is on q, not on the rounded root)
// A non-negative float's bit pattern is order-preserving, so min and argmin are ONE unsigned 64-bit minimum of (bits(q) << 32) | j:
// integer minima, which have no order to promise.  With no admissible j (nb == 1 with the diagonal excluded) the row gets sum = 0, min =
// +inf, argmin = 0xFFFFFFFF.  A NaN or +-inf element in row i of a makes that row's outputs NaN, NaN, 0xFFFFFFFF and touches no other
// row; a NaN or +-inf element anywhere in b does the same to every row.  Both come from flags taken while the tables are staged, never
// from inf - inf.  Finite elements whose t_c or q overflows float32 follow IEEE from there: dist = inf, and ties at inf go to the
// smallest j like any other tie.
//
// THE ORDER of the float64 sum of row i, which is one order for both forms (so the forms agree bit for bit):
//   * the rows of b are cut into tiles of T = 32; the tiles into SEGMENTS of G = 16 tiles (d3p_pair_stats_segment_tiles); within a
//     segment tile J belongs to SLOT J mod 4;
//   * one wavefront computes a 32 x 32 pair tile (I, J): lane l = 8 ti + tj owns the 4 x 4 pairs (i, j) = (32 I + ti + 8 ki, 32 J + tj +
//     8 kj).  For each ki it adds the dist of its pairs in the order kj = 0 .. 3 onto ONE float64 sum, over the slot's tiles of the
//     segment in ascending J, from 0 (a pair that is not admissible adds +0.0, which changes no bit of a non-negative sum);
//   * the 8 lanes tj = 0 .. 7 of a row are summed by the xor butterfly 4, 2, 1 (a + b is commutative: the 8 lanes end with equal bits):
//     the slot sum of row i;
//   * per segment the four slot sums are added in ascending order onto 0, and the segments are added in ascending order onto 0.
// The wide form (1) gives one workgroup one tile of a: its four wavefronts are the slots and walk every segment, the slots meet in LDS
// after each segment, and nothing else is needed.  The split form (2) gives a workgroup one tile of a and ONE segment and writes, per
// (segment, row), the segment's float64 sum, its packed minimum and its flags to the caller's buffer; a second launch adds them in
// ascending segment order.  Every (segment, row < na) cell is written before it is read: the buffer's contents on entry change nothing.
// Either form stages the two sides of a pair tile in chunks of C = 32 columns in its wavefront's own LDS (2 x 32 x 36 floats; the row
// stride 36 keeps the 16-byte reads of the 8 distinct rows of a quarter wave on distinct banks), so neither table's length nor d is
// bounded by LDS; the pair accumulators q stay in registers across the chunks, which keeps the chain's order.  A chunk is padded with
// zeros to a multiple of 4 columns: fmaf(0, 0, q) = q for every q >= 0, NaN or inf.  Static LDS: 40464 bytes.  No floating-point
// atomics (no atomics at all), no host synchronisation, no dynamic LDS, no scratch.
//
// DETERMINISM.  Repeated calls give equal bits.  The three outputs of row i depend on that row's values, the table b, nb, d and the flag
// alone: not on na, the other rows of a, a_ld, b_ld, the row's place in its tile, the form, or what the buffer held before.
//
// Distances are NOT taken from a Gram matrix (|a|^2 + |b|^2 - 2 a.b): for records that sit close together far from the origin the
// cancellation loses every digit of the distance, and the nearest record is exactly where that happens.
#include "d3p_device.h"
#include "d3p_host.h"
#include "d3p_pair_tile.h"

#define D3P_PS_G 16          // tiles of b per segment (a multiple of the slots)
#define D3P_PS_FORM_WIDE 1
#define D3P_PS_FORM_SPLIT 2
#define D3P_PS_WIDE_MIN_TILES 1024u  // the wide form is chosen where the tiles of a alone fill the chip: 256 CUs x 4 resident workgroups
#define D3P_PS_NONE 0xFFFFFFFFFFFFFFFFull
#define D3P_PS_CELL 20u      // bytes per (segment, row) of the split form: a double, a packed minimum, a flag word

static int32_t g_ps_form = 0;   // d3p_pair_stats_set_form: 0 = the rule below

namespace d3p {

struct PsArgs {
    const uint32_t* a; const uint32_t* b; int32_t dtype; int64_t a_ld, b_ld; uint32_t na, nb, d, excl, nseg;
    double* sum; float* min; uint32_t* argmin;
    double* ws_sum; unsigned long long* ws_min; uint32_t* ws_flag;
};

// the items of one table: its n rows
struct PsItems {
    typedef uint64_t index;
    const uint32_t* base; int64_t ld; uint32_t n;
    __device__ __forceinline__ bool live(uint64_t row) const { return row < n; }
    __device__ __forceinline__ uint32_t word(uint64_t row, uint32_t col) const { return base[(int64_t)row * ld + col]; }
};

// the IEEE root.  sqrtf is correctly rounded under the compiler's default -fhip-fp32-correctly-rounded-divide-sqrt; the rounded-root
// intrinsic of this toolchain's headers is the NATIVE instruction (1 ulp) unless OCML_BASIC_ROUNDED_OPERATIONS is defined, which the
// by-value tests of non-square q tell apart
__device__ __forceinline__ float ps_sqrt(float q) { return __builtin_sqrtf(q); }

// the tiles of one slot of one segment against tile I of a: adds onto the lane's four sums, lowers its four packed minima, ors bad_b.
// With a_resident (d <= C) tile I of a already lies in A.
__device__ __forceinline__ void ps_segment_slot(const PsArgs& a, uint32_t I, uint32_t seg, uint32_t slot, float* A, float* B, uint32_t* aflag,
                                                bool a_resident, int lane, double (&ls)[4], unsigned long long (&pm)[4], bool& bad_b)
{
    const uint32_t ntb = (uint32_t)(((uint64_t)a.nb + D3P_PAIR_T - 1u) / D3P_PAIR_T);
    const uint32_t j_lo = seg * D3P_PS_G, j_hi = ntb - j_lo < D3P_PS_G ? ntb : j_lo + D3P_PS_G;
    const uint32_t ti = (uint32_t)lane >> 3, tj = (uint32_t)lane & 7u;
    bool bad_a = false;   // (the rows' flags go to aflag)
    const PsItems rows_a = {a.a, a.a_ld, a.na}, rows_b = {a.b, a.b_ld, a.nb};
    for (uint32_t J = j_lo + slot; J < j_hi; J += D3P_PAIR_WAVES) {
        float q[4][4];
        pair_zero(q);
        for (uint32_t c0 = 0; c0 < a.d; c0 += D3P_PAIR_C) {
            const uint32_t cw = a.d - c0 < D3P_PAIR_C ? a.d - c0 : D3P_PAIR_C;
            const int lw = pair_lanes_log2(cw);
            {
                uint32_t wa[16], wb[16];
                if (!a_resident) pair_load(rows_a, I, c0, cw, lw, lane, wa);
                pair_load(rows_b, J, c0, cw, lw, lane, wb);
                pair_wave_sync();   // the reads of the chunk before are done
                if (!a_resident) pair_store(a.dtype, A, aflag, lw, lane, wa, bad_a);
                pair_store(a.dtype, B, nullptr, lw, lane, wb, bad_b);
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
        for (int ki = 0; ki < 4; ++ki) {
            const uint64_t i = (uint64_t)I * D3P_PAIR_T + ti + 8u * ki;
#pragma unroll
            for (int kj = 0; kj < 4; ++kj) {
                const uint64_t j = (uint64_t)J * D3P_PAIR_T + tj + 8u * kj;
                const bool ok = j < a.nb && !(a.excl && j == i);
                const float qv = q[ki][kj];
                const double dist = (double)ps_sqrt(qv);
                ls[ki] += ok ? dist : 0.0;
                const unsigned long long key = ((unsigned long long)__float_as_uint(qv) << 32) | (unsigned long long)j;
                pm[ki] = ok && key < pm[ki] ? key : pm[ki];
            }
        }
    }
}

__device__ __forceinline__ double ps_row_sum(double v)
{
    for (int off = 4; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ unsigned long long ps_row_min(unsigned long long v)
{
    for (int off = 4; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// the three outputs of row i from its float64 sum, its packed minimum and its flags
__device__ __forceinline__ void ps_finish(const PsArgs& a, uint64_t i, double total, unsigned long long key, bool bad)
{
    const float nan = __builtin_nanf("");
    const bool none = key == D3P_PS_NONE;
    a.sum[i] = bad ? (double)nan : total;
    a.min[i] = bad ? nan : none ? __builtin_inff() : ps_sqrt(__uint_as_float((uint32_t)(key >> 32)));
    a.argmin[i] = bad || none ? 0xFFFFFFFFu : (uint32_t)(key & 0xFFFFFFFFull);
}

template <int FORM>
__global__ __launch_bounds__(64 * D3P_PAIR_WAVES) void k_pair_stats(PsArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[D3P_PAIR_WAVES][2][D3P_PAIR_T * D3P_PAIR_LD];
    __shared__ double slot_sum[2][D3P_PAIR_WAVES][D3P_PAIR_T];
    __shared__ unsigned long long slot_min[D3P_PAIR_WAVES][D3P_PAIR_T];
    __shared__ uint32_t slot_aflag[D3P_PAIR_WAVES][D3P_PAIR_T];
    __shared__ uint32_t slot_bflag[D3P_PAIR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ti = (uint32_t)lane >> 3, tj = (uint32_t)lane & 7u;
    float* A = lds[wave][0];
    float* B = lds[wave][1];
    uint32_t* aflag = slot_aflag[wave];
    const uint32_t I = FORM == D3P_PS_FORM_WIDE ? blockIdx.x : blockIdx.x / a.nseg;
    const uint32_t seg_lo = FORM == D3P_PS_FORM_WIDE ? 0u : blockIdx.x % a.nseg;
    const uint32_t seg_hi = FORM == D3P_PS_FORM_WIDE ? a.nseg : seg_lo + 1u;
    if (lane < D3P_PAIR_T) aflag[lane] = 0u;
    pair_wave_sync();
    const bool a_resident = a.d <= D3P_PAIR_C;
    bool bad_b = false;
    if (a_resident) {   // one chunk: tile I of a is staged once, by every wavefront for itself
        const int lw = pair_lanes_log2(a.d);
        uint32_t wa[16];
        bool bad_a = false;
        pair_load(PsItems{a.a, a.a_ld, a.na}, I, 0u, a.d, lw, lane, wa);
        pair_store(a.dtype, A, aflag, lw, lane, wa, bad_a);
        pair_wave_sync();
    }
    unsigned long long pm[4] = {D3P_PS_NONE, D3P_PS_NONE, D3P_PS_NONE, D3P_PS_NONE};
    double total = 0.0;   // (threads 0 .. 31: row 32 I + threadIdx.x)
    for (uint32_t seg = seg_lo; seg < seg_hi; ++seg) {
        double ls[4] = {0.0, 0.0, 0.0, 0.0};
        ps_segment_slot(a, I, seg, (uint32_t)wave, A, B, aflag, a_resident, lane, ls, pm, bad_b);
        const uint32_t par = seg & 1u;
#pragma unroll
        for (int ki = 0; ki < 4; ++ki) {
            const double s = ps_row_sum(ls[ki]);
            if (tj == 0) slot_sum[par][wave][ti + 8u * ki] = s;
        }
        // one barrier per segment: the sums of segment s + 2 are written after the barrier of segment s + 1, which follows the reads below
        __syncthreads();
        if (threadIdx.x < D3P_PAIR_T) {
            double s = 0.0;
            for (int w = 0; w < D3P_PAIR_WAVES; ++w) s += slot_sum[par][w][threadIdx.x];
            total += s;
        }
    }
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
        const unsigned long long m = ps_row_min(pm[ki]);
        if (tj == 0) slot_min[wave][ti + 8u * ki] = m;
    }
    bad_b = __builtin_amdgcn_ballot_w64(bad_b) != 0ull;
    if (lane == 0) slot_bflag[wave] = bad_b ? 1u : 0u;
    __syncthreads();
    if (threadIdx.x < D3P_PAIR_T) {
        const uint64_t i = (uint64_t)I * D3P_PAIR_T + threadIdx.x;
        if (i < a.na) {
            unsigned long long key = D3P_PS_NONE;
            uint32_t fa = 0u, fb = 0u;
            for (int w = 0; w < D3P_PAIR_WAVES; ++w) {
                key = slot_min[w][threadIdx.x] < key ? slot_min[w][threadIdx.x] : key;
                fa |= slot_aflag[w][threadIdx.x];
                fb |= slot_bflag[w];
            }
            if (FORM == D3P_PS_FORM_WIDE) {
                ps_finish(a, i, total, key, (fa | fb) != 0u);
            } else {
                const uint64_t cell = (uint64_t)seg_lo * a.na + i;
                a.ws_sum[cell] = total;
                a.ws_min[cell] = key;
                a.ws_flag[cell] = fa | (fb << 1);
            }
        }
    }
}

// the split form's second launch: one thread per row adds its cells in ascending segment order
__global__ __launch_bounds__(256) void k_pair_stats_merge(PsArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.na) return;
    double total = 0.0;
    unsigned long long key = D3P_PS_NONE;
    uint32_t flags = 0u;
    for (uint32_t seg = 0; seg < a.nseg; ++seg) {
        const uint64_t cell = (uint64_t)seg * a.na + i;
        total += a.ws_sum[cell];
        key = a.ws_min[cell] < key ? a.ws_min[cell] : key;
        flags |= a.ws_flag[cell];
    }
    ps_finish(a, i, total, key, flags != 0u);
}

static uint32_t ps_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + D3P_PAIR_T - 1u) / D3P_PAIR_T); }

static uint32_t ps_segments(uint32_t nb) { return (ps_tiles(nb) + D3P_PS_G - 1u) / D3P_PS_G; }

static uint32_t ps_form(uint32_t na, uint32_t nb, uint32_t d)
{
    if (na < 1 || nb < 1 || d < 1) return 0;
    if (g_ps_form) return (uint32_t)g_ps_form;
    // the split form where the tiles of a alone cannot fill the chip and b has more than one segment to deal out; the forms agree bit
    // for bit, so the choice may look at na
    return ps_tiles(na) < D3P_PS_WIDE_MIN_TILES && ps_segments(nb) > 1u ? D3P_PS_FORM_SPLIT : D3P_PS_FORM_WIDE;
}

static size_t ps_workspace(uint32_t na, uint32_t nb, uint32_t d)
{
    if (ps_form(na, nb, d) != D3P_PS_FORM_SPLIT) return 0;
    return (size_t)ps_segments(nb) * (size_t)na * D3P_PS_CELL;   // < 2^23 x 2^32 x 20: no wrap
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_pair_stats_tile_rows(void) { return D3P_PAIR_T; }

uint32_t d3p_pair_stats_chunk_cols(void) { return D3P_PAIR_C; }

uint32_t d3p_pair_stats_segment_tiles(void) { return D3P_PS_G; }

uint32_t d3p_pair_stats_form(uint32_t na, uint32_t nb, uint32_t d) { return ps_form(na, nb, d); }

size_t d3p_pair_stats_workspace(uint32_t na, uint32_t nb, uint32_t d) { return ps_workspace(na, nb, d); }

int d3p_pair_stats_set_form(int32_t form)
{
    if (form != 0 && form != D3P_PS_FORM_WIDE && form != D3P_PS_FORM_SPLIT)
        return fail(D3P_E_INVALID_ARG, "d3p_pair_stats_set_form: form must be 0 (the rule), 1 (wide) or 2 (split), got %d", form);
    g_ps_form = form;
    return D3P_OK;
}

int d3p_pair_stats(void* stream, const void* a_dev, const void* b_dev, int32_t dtype, int64_t a_ld, int64_t b_ld, uint32_t na, uint32_t nb,
                   uint32_t d, int32_t exclude_diagonal, double* sum_dev, float* min_dev, uint32_t* argmin_dev, void* ws_dev, size_t ws_bytes)
{
    const char* what = "d3p_pair_stats";
    if (!a_dev || !b_dev || !sum_dev || !min_dev || !argmin_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)a_dev | (uintptr_t)b_dev | (uintptr_t)min_dev | (uintptr_t)argmin_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if ((((uintptr_t)sum_dev | (uintptr_t)ws_dev) & 7u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: sum_dev or ws_dev is not aligned to 8 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (na < 1 || nb < 1) return fail(D3P_E_INVALID_ARG, "%s: na >= 1 and nb >= 1 are required", what);
    if (d < 1) return fail(D3P_E_INVALID_ARG, "%s: d >= 1 is required", what);
    if (a_ld < 0 || (uint64_t)a_ld < d) return fail(D3P_E_INVALID_ARG, "%s: a_ld >= d is required", what);
    if (b_ld < 0 || (uint64_t)b_ld < d) return fail(D3P_E_INVALID_ARG, "%s: b_ld >= d is required", what);
    if ((uint64_t)na > (uint64_t)INT64_MAX / (uint64_t)a_ld || (uint64_t)nb > (uint64_t)INT64_MAX / (uint64_t)b_ld)
        return fail(D3P_E_INVALID_ARG, "%s: na * a_ld or nb * b_ld does not fit 63 bits", what);
    if (exclude_diagonal != 0 && exclude_diagonal != 1)
        return fail(D3P_E_INVALID_ARG, "%s: exclude_diagonal must be 0 or 1, got %d", what, exclude_diagonal);
    if (exclude_diagonal && na != nb)
        return fail(D3P_E_INVALID_ARG, "%s: exclude_diagonal compares a table with itself: na == nb is required (%u, %u)", what, na, nb);
    const uint32_t form = ps_form(na, nb, d);
    const size_t need = ps_workspace(na, nb, d);
    if (ws_bytes < need || (need && !ws_dev))
        return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_dev ? ws_bytes : (size_t)0, need);
    const uint64_t groups = (uint64_t)ps_tiles(na) * (form == D3P_PS_FORM_SPLIT ? ps_segments(nb) : 1u);
    if (groups > 0x7fffffffull) return fail(D3P_E_UNSUPPORTED, "%s: more than 2^31 - 1 workgroups (one per tile of a and segment of b)", what);
    if (!is_device_ptr(a_dev) || !is_device_ptr(b_dev) || !is_device_ptr(sum_dev) || !is_device_ptr(min_dev) || !is_device_ptr(argmin_dev) ||
        (need && !is_device_ptr(ws_dev)))
        return fail(D3P_E_INVALID_ARG, "%s: the tables, the outputs and the workspace must be device memory", what);
    PsArgs a;
    a.a = static_cast<const uint32_t*>(a_dev); a.b = static_cast<const uint32_t*>(b_dev); a.dtype = dtype; a.a_ld = a_ld; a.b_ld = b_ld;
    a.na = na; a.nb = nb; a.d = d; a.excl = (uint32_t)exclude_diagonal; a.nseg = ps_segments(nb);
    a.sum = sum_dev; a.min = min_dev; a.argmin = argmin_dev;
    const size_t cells = (size_t)a.nseg * na;
    a.ws_sum = static_cast<double*>(ws_dev);
    a.ws_min = need ? reinterpret_cast<unsigned long long*>(static_cast<char*>(ws_dev) + 8u * cells) : nullptr;
    a.ws_flag = need ? reinterpret_cast<uint32_t*>(static_cast<char*>(ws_dev) + 16u * cells) : nullptr;
    if (form == D3P_PS_FORM_WIDE) {
        hipLaunchKernelGGL(k_pair_stats<D3P_PS_FORM_WIDE>, dim3((unsigned)groups), dim3(64 * D3P_PAIR_WAVES), 0, (hipStream_t)stream, a);
        return check_launch(what);
    }
    hipLaunchKernelGGL(k_pair_stats<D3P_PS_FORM_SPLIT>, dim3((unsigned)groups), dim3(64 * D3P_PAIR_WAVES), 0, (hipStream_t)stream, a);
    const int rc = check_launch(what);
    if (rc != D3P_OK) return rc;
    hipLaunchKernelGGL(k_pair_stats_merge, dim3((unsigned)(((uint64_t)na + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch(what);
}

}  // extern "C"
