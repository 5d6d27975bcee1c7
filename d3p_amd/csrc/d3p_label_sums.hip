// Label sums of the pooled pair distances (d3p_amd/permutation.py, include/d3p_hip.h): for R labellings g_r of the m pooled
// rows of a table z the quadratic form s11[r] = sum_{i,j} g_i g_j D_ij of the distance matrix D, which is all that a relabelling of the
// two-sample energy distance needs of the pairs -- the permutation test of Szekely & Rizzo in ONE walk that computes every distance once
// and feeds it to every labelling while it lies in LDS; never the m x m matrix, never a walk per labelling.  The entry
// d3p_pair_label_sums with its host checks, its two kernels and the query functions of their constants and workspace.
//
// THE RULE.  z[i * ld + c] is pooled row i < m in column c < d, float32 (dtype 0) or int32 (dtype 1: converted to float32 when staged,
// exact for |v| <= 2^24, which is what the Python layer admits).  D_ij is the distance of d3p_pair_stats.hip, bit for bit:
//     t_c = fl32(z_ic - z_jc)      q = the float32 fmaf chain q <- fmaf(t_c, t_c, q) over c = 0 .. d-1 ascending, from q = 0
//     D_ij = sqrtf(q), correctly rounded (the IEEE root: ls_sqrt below, not the native instruction's 1 ulp)
// by the tile and the chain of d3p_pair_tile.h; D_ii is exactly +0.0 and D_ij == D_ji bitwise.  labels[tile * R + r] is a uint32 whose bit
// p says that row 32 tile + p carries label 1 in labelling r (tile-major: adjacent labellings are adjacent words).  Bits of rows >= m in
// the last tile's words are IGNORED, whatever they hold; the words are only ever read as bits, never as an index.  With g_i the live bit:
//     s11[r] = sum_{i,j} g_i g_j (double)D_ij      in float64, in the order below, not rounded further
//     s1t[r] = sum_i g_i row_sum[i]                over i ascending onto 0 (a row that is not selected adds nothing)
//     n1[r]  = the population count of the live bits
// row_sum is the caller's (pair_stats(z, z, exclude_diagonal)["sum"]); s1t propagates what it holds on the selected rows.  A NaN or +-inf
// element anywhere in z makes EVERY s11[r] NaN: from the flag taken while the table is staged, never from inf - inf (every workgroup
// stages every row, so every workgroup knows).  Finite elements whose t_c or q overflows float32 follow IEEE from there: D_ij = inf, and
// s11[r] = inf where such a pair is selected.
//
// THE ORDER of s11[r], which is ONE order (there is one form):
//   * the pooled rows are cut into tiles of T = 32; tile J belongs to SLOT J mod 4;
//   * per (tile pair (I, J), labelling r) and row ii = 0 .. 31 of tile I: the ROW SUM adds (double)D[ii][jj] for jj = 0 .. 31 ascending
//     onto 0, a pair whose column bit is clear adding +0.0 (by select, which changes no bit of a non-negative sum);
//   * per (I, slot, r) the SLOT SUM adds the row sums whose row bit is set (a clear one adds +0.0) in the order ii ascending within a
//     tile pair and J ascending over the slot's tiles, onto 0;
//   * per (I, r) the four slot sums are added in ascending order onto 0: the CELL (I, r), a float64 of the caller's workspace;
//   * s11[r] adds the cells in ascending I onto 0 (the second launch).
// The longest chain of float64 additions is A = 32 + 32 ceil(tiles / 4) + 4 + tiles.
// A workgroup of four wavefronts (the slots) owns one tile I and one BLOCK of 8 x 64 = 512 consecutive labellings
// (d3p_pair_label_sums_block_labellings); blocks are independent, so s11[r] does not see R.  Phase 1: the wavefront computes the 32 x 32
// tile of q as k_pair_stats does (lane 8 ti + tj, 4 x 4 pairs, chunks of C = 32 columns staged in its own 2 x 32 x 36 floats), roots it
// and writes the 1024 float32 distances to 4 KiB of its own LDS.  Phase 2: lanes become labellings; lane l of group k holds the words
// (I, r) and (J, r) of labelling r = 512 block + 64 k + l, every lane reads the same distance (an LDS broadcast) and adds it under its
// own bits.  The slots meet in the distance buffers, which are dead by then.  Static LDS: 53264 bytes.  No floating-point atomics (no
// atomics at all), no host synchronisation, no dynamic LDS, no scratch.  Every cell (I, r < R) is written before it is read: the
// workspace's contents on entry change nothing.
//
// DETERMINISM.  Repeated calls give equal bits.  s11[r] depends on z, m, d and labelling r alone: not on R, the other labellings, r's
// place in its group of 64 or its block, ld, or what the workspace held before.
#include "d3p_device.h"
#include "d3p_host.h"
#include "d3p_pair_tile.h"

#define D3P_LS_GROUPS 8u                      // groups of 64 labellings per block: their sums stay in registers
#define D3P_LS_BLOCK (64u * D3P_LS_GROUPS)    // labellings per workgroup
#define D3P_LS_MAX_R 65536u                   // the cap on R (d3p_pair_label_sums_max_labellings)

namespace d3p {

struct LsArgs {
    const uint32_t* z; int32_t dtype; int64_t ld; uint32_t m, d, R, ntiles, nblocks;
    const uint32_t* labels; const double* row_sum;
    double* s11; double* s1t; uint32_t* n1; double* cells;
};

// the items of the pooled table: its m rows
struct LsItems {
    typedef uint64_t index;
    const uint32_t* base; int64_t ld; uint32_t n;
    __device__ __forceinline__ bool live(uint64_t row) const { return row < n; }
    __device__ __forceinline__ uint32_t word(uint64_t row, uint32_t col) const { return base[(int64_t)row * ld + col]; }
};

// the IEEE root, as d3p_pair_stats.hip takes it (correctly rounded under the compiler's default; the rounded-root intrinsic of this
// toolchain's headers is the 1 ulp instruction)
__device__ __forceinline__ float ls_sqrt(float q) { return __builtin_sqrtf(q); }

// the bits of the rows of `tile` that exist
__device__ __forceinline__ uint32_t ls_live_bits(uint32_t tile, uint32_t m)
{
    const uint64_t lo = (uint64_t)tile * D3P_PAIR_T;
    return lo + D3P_PAIR_T <= m ? 0xFFFFFFFFu : lo >= m ? 0u : (1u << (uint32_t)(m - lo)) - 1u;
}

__device__ __forceinline__ double ls_pick(uint32_t word, uint32_t bit, float v) { return (double)(((word >> bit) & 1u) ? v : 0.0f); }

__global__ __launch_bounds__(64 * D3P_PAIR_WAVES) void k_pair_label_sums(LsArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[D3P_PAIR_WAVES][2][D3P_PAIR_T * D3P_PAIR_LD];
    __shared__ __attribute__((aligned(16))) float dist_lds[D3P_PAIR_WAVES][D3P_PAIR_T * D3P_PAIR_T];   // (= 512 doubles: a slot's sums)
    __shared__ uint32_t slot_flag[D3P_PAIR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ti = (uint32_t)lane >> 3, tj = (uint32_t)lane & 7u;
    float* A = lds[wave][0];
    float* B = lds[wave][1];
    float* D = dist_lds[wave];
    const uint32_t I = blockIdx.x / a.nblocks, block = blockIdx.x % a.nblocks;
    const uint32_t r0 = block * D3P_LS_BLOCK;
    const uint32_t left = a.R - r0;
    const uint32_t ng = left >= D3P_LS_BLOCK ? D3P_LS_GROUPS : (left + 63u) / 64u;   // live groups of this block, >= 1
    const LsItems rows = {a.z, a.ld, a.m};
    const bool a_resident = a.d <= D3P_PAIR_C;
    bool bad = false;
    if (a_resident) {   // one chunk: tile I is staged once, by every wavefront for itself
        const int lw = pair_lanes_log2(a.d);
        uint32_t wa[16];
        pair_load(rows, I, 0u, a.d, lw, lane, wa);
        pair_store(a.dtype, A, nullptr, lw, lane, wa, bad);
        pair_wave_sync();
    }
    // the words of tile I: lane l of group k is labelling r0 + 64 k + l (none beyond R: all bits clear)
    uint32_t wi[D3P_LS_GROUPS];
    const uint32_t live_i = ls_live_bits(I, a.m);
#pragma unroll
    for (uint32_t k = 0; k < D3P_LS_GROUPS; ++k) {
        const uint32_t r = r0 + 64u * k + (uint32_t)lane;
        wi[k] = k < ng && r < a.R ? a.labels[(size_t)I * a.R + r] & live_i : 0u;
    }
    double acc[D3P_LS_GROUPS];
#pragma unroll
    for (uint32_t k = 0; k < D3P_LS_GROUPS; ++k) acc[k] = 0.0;
    for (uint32_t J = (uint32_t)wave; J < a.ntiles; J += D3P_PAIR_WAVES) {
        uint32_t wj[D3P_LS_GROUPS];
        const uint32_t live_j = ls_live_bits(J, a.m);
#pragma unroll
        for (uint32_t k = 0; k < D3P_LS_GROUPS; ++k) {
            const uint32_t r = r0 + 64u * k + (uint32_t)lane;
            wj[k] = k < ng && r < a.R ? a.labels[(size_t)J * a.R + r] & live_j : 0u;
        }
        // phase 1: the 32 x 32 tile of q, as k_pair_stats computes it
        float q[4][4];
        pair_zero(q);
        for (uint32_t c0 = 0; c0 < a.d; c0 += D3P_PAIR_C) {
            const uint32_t cw = a.d - c0 < D3P_PAIR_C ? a.d - c0 : D3P_PAIR_C;
            const int lw = pair_lanes_log2(cw);
            {
                uint32_t wa[16], wb[16];
                if (!a_resident) pair_load(rows, I, c0, cw, lw, lane, wa);
                pair_load(rows, J, c0, cw, lw, lane, wb);
                pair_wave_sync();   // the reads of the chunk before are done
                if (!a_resident) pair_store(a.dtype, A, nullptr, lw, lane, wa, bad);
                pair_store(a.dtype, B, nullptr, lw, lane, wb, bad);
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
            for (int kj = 0; kj < 4; ++kj) D[(ti + 8u * ki) * D3P_PAIR_T + tj + 8u * kj] = ls_sqrt(q[ki][kj]);
        pair_wave_sync();
        // phase 2: lanes are labellings; every lane reads the same 32 distances of row ii
        for (uint32_t ii = 0; ii < D3P_PAIR_T; ++ii) {
            float4 v[D3P_PAIR_T / 4];
#pragma unroll
            for (uint32_t k4 = 0; k4 < D3P_PAIR_T / 4; ++k4) v[k4] = *reinterpret_cast<const float4*>(D + ii * D3P_PAIR_T + 4u * k4);
#pragma unroll
            for (uint32_t k = 0; k < D3P_LS_GROUPS; ++k) {
                if (k < ng) {
                    const uint32_t w = wj[k];
                    double row = 0.0;
#pragma unroll
                    for (uint32_t k4 = 0; k4 < D3P_PAIR_T / 4; ++k4) {
                        row += ls_pick(w, 4u * k4, v[k4].x);
                        row += ls_pick(w, 4u * k4 + 1u, v[k4].y);
                        row += ls_pick(w, 4u * k4 + 2u, v[k4].z);
                        row += ls_pick(w, 4u * k4 + 3u, v[k4].w);
                    }
                    acc[k] += ((wi[k] >> ii) & 1u) ? row : 0.0;
                }
            }
        }
        pair_wave_sync();   // the distances are read before the next tile's are written
    }
    // the slots meet: a wavefront's 512 sums take the place of its distances
    double* mine = reinterpret_cast<double*>(D);
#pragma unroll
    for (uint32_t k = 0; k < D3P_LS_GROUPS; ++k) mine[64u * k + (uint32_t)lane] = acc[k];
    bad = __builtin_amdgcn_ballot_w64(bad) != 0ull;
    if (lane == 0) slot_flag[wave] = bad ? 1u : 0u;
    __syncthreads();
    uint32_t flags = 0u;
    for (int w = 0; w < D3P_PAIR_WAVES; ++w) flags |= slot_flag[w];
    for (uint32_t t = threadIdx.x; t < D3P_LS_BLOCK; t += 64u * D3P_PAIR_WAVES) {
        const uint32_t r = r0 + t;
        if (r < a.R) {
            double s = 0.0;
            for (int w = 0; w < D3P_PAIR_WAVES; ++w) s += reinterpret_cast<const double*>(dist_lds[w])[t];
            a.cells[(size_t)I * a.R + r] = flags ? (double)__builtin_nanf("") : s;
        }
    }
}

// the second launch: one thread per labelling adds its cells in ascending tile order, and walks its words for s1t and n1
__global__ __launch_bounds__(256) void k_pair_label_sums_merge(LsArgs a)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.R) return;
    double s = 0.0, t = 0.0;
    uint32_t n = 0u;
    for (uint32_t tile = 0; tile < a.ntiles; ++tile) {
        s += a.cells[(size_t)tile * a.R + r];
        const uint32_t w = a.labels[(size_t)tile * a.R + r] & ls_live_bits(tile, a.m);
        const uint64_t lo = (uint64_t)tile * D3P_PAIR_T;
        const uint32_t rows = a.m - lo < D3P_PAIR_T ? (uint32_t)(a.m - lo) : D3P_PAIR_T;
        for (uint32_t p = 0; p < rows; ++p) {
            const double v = a.row_sum[lo + p];
            if ((w >> p) & 1u) t += v;
        }
        n += (uint32_t)__builtin_popcount(w);
    }
    a.s11[r] = s;
    a.s1t[r] = t;
    a.n1[r] = n;
}

static uint32_t ls_tiles(uint32_t m) { return (uint32_t)(((uint64_t)m + D3P_PAIR_T - 1u) / D3P_PAIR_T); }

static bool ls_shape_ok(uint32_t m, uint32_t d, uint32_t R) { return m >= 1 && d >= 1 && R >= 1 && R <= D3P_LS_MAX_R; }

static size_t ls_workspace(uint32_t m, uint32_t d, uint32_t R)
{
    if (!ls_shape_ok(m, d, R)) return 0;
    return (size_t)ls_tiles(m) * (size_t)R * sizeof(double);   // < 2^27 x 2^16 x 8: no wrap
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_pair_label_sums_tile_rows(void) { return D3P_PAIR_T; }

uint32_t d3p_pair_label_sums_block_labellings(void) { return D3P_LS_BLOCK; }

uint32_t d3p_pair_label_sums_max_labellings(void) { return D3P_LS_MAX_R; }

size_t d3p_pair_label_sums_workspace(uint32_t m, uint32_t d, uint32_t R) { return ls_workspace(m, d, R); }

int d3p_pair_label_sums(void* stream, const void* z_dev, int32_t dtype, int64_t ld, uint32_t m, uint32_t d, uint32_t R,
                        const uint32_t* labels_dev, const double* row_sum_dev, double* s11_dev, double* s1t_dev, uint32_t* n1_dev,
                        void* ws_dev, size_t ws_bytes)
{
    const char* what = "d3p_pair_label_sums";
    const size_t need = ls_workspace(m, d, R);
    if (!z_dev || !labels_dev || !row_sum_dev || !s11_dev || !s1t_dev || !n1_dev || (need && !ws_dev))
        return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)z_dev | (uintptr_t)labels_dev | (uintptr_t)n1_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if ((((uintptr_t)row_sum_dev | (uintptr_t)s11_dev | (uintptr_t)s1t_dev | (uintptr_t)ws_dev) & 7u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: row_sum_dev, s11_dev, s1t_dev or ws_dev is not aligned to 8 bytes", what);
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (m < 1) return fail(D3P_E_INVALID_ARG, "%s: m >= 1 is required", what);
    if (d < 1) return fail(D3P_E_INVALID_ARG, "%s: d >= 1 is required", what);
    if (ld < 0 || (uint64_t)ld < d) return fail(D3P_E_INVALID_ARG, "%s: ld >= d is required", what);
    if ((uint64_t)m > (uint64_t)INT64_MAX / (uint64_t)ld) return fail(D3P_E_INVALID_ARG, "%s: m * ld does not fit 63 bits", what);
    if (R < 1 || R > D3P_LS_MAX_R)
        return fail(D3P_E_INVALID_ARG, "%s: 1 <= R <= %u labellings are required, got %u", what, D3P_LS_MAX_R, R);
    const uint32_t ntiles = ls_tiles(m), nblocks = (R + D3P_LS_BLOCK - 1u) / D3P_LS_BLOCK;
    const uint64_t groups = (uint64_t)ntiles * nblocks;
    if (groups > 0x7fffffffull)
        return fail(D3P_E_UNSUPPORTED, "%s: %u tiles of rows x %u blocks of labellings = %llu workgroups, more than 2^31 - 1", what, ntiles,
                    nblocks, (unsigned long long)groups);
    if (ws_bytes < need) return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_bytes, need);
    if (!is_device_ptr(z_dev) || !is_device_ptr(labels_dev) || !is_device_ptr(row_sum_dev) || !is_device_ptr(s11_dev) ||
        !is_device_ptr(s1t_dev) || !is_device_ptr(n1_dev) || !is_device_ptr(ws_dev))
        return fail(D3P_E_INVALID_ARG, "%s: the table, the labels, the row sums, the outputs and the workspace must be device memory", what);
    LsArgs a;
    a.z = static_cast<const uint32_t*>(z_dev); a.dtype = dtype; a.ld = ld; a.m = m; a.d = d; a.R = R; a.ntiles = ntiles; a.nblocks = nblocks;
    a.labels = labels_dev; a.row_sum = row_sum_dev; a.s11 = s11_dev; a.s1t = s1t_dev; a.n1 = n1_dev; a.cells = static_cast<double*>(ws_dev);
    hipLaunchKernelGGL(k_pair_label_sums, dim3((unsigned)groups), dim3(64 * D3P_PAIR_WAVES), 0, (hipStream_t)stream, a);
    const int rc = check_launch(what);
    if (rc != D3P_OK) return rc;
    hipLaunchKernelGGL(k_pair_label_sums_merge, dim3((R + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch(what);
}

}  // extern "C"
