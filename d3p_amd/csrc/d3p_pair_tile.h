// The wavefront-private 32 x 32 tile of squared distances and what its four walkers share, one definition each: the energy score
// (d3p_energy.hip), the pair statistics (d3p_pair_stats.hip, 4w), the label sums (d3p_label_sums.hip, 4y) and the k
// nearest neighbours (d3p_pair_knn.hip, 4za).  The tile's constants, the wave sync of its LDS, the lane -> (item, column) map of a
// staged chunk with its load and store, and the chain
//     t_c = fl32(a_c - b_c)      q <- fmaf(t_c, t_c, q)      over c ascending
// of one pair over four columns.  A wavefront stages C = 32 columns of the 32 items of each side in its own 2 x 32 x 36 floats of LDS
// (load -> wave sync -> store -> wave sync); lane 8 ti + tj keeps the 4 x 4 pairs (ti + 8 ki, tj + 8 kj) in registers across the chunks
// and reads its 4 + 4 rows 16 bytes at a time.  Beside them: the rows of a table as items, the root, the tile count, the eight-lane row
// reduction, the resident prologue, the admissible pairs and their packed key, the (tile, segment) dispatch of the split form, and
// -- HOST, at the end -- the form rule, the split form's two launches and the refusals that the entries share.  The walk over tiles,
// slots and segments, the staging of a chunk (its sides differ: the energy score's diagonal tiles stage one), the column loop over a
// chunk (a dozen lines: as a helper it cost a wave of occupancy, docs/experiments_fidelity.md) and the epilogues stay their files' own.
#pragma once
#include "d3p_device.h"

#define D3P_PAIR_T 32          // items per side of a pair tile
#define D3P_PAIR_C 32          // columns per staged chunk
#define D3P_PAIR_LD 36         // LDS row stride in floats (a multiple of 4: the reads are 16 bytes wide)
#define D3P_PAIR_WAVES 4       // wavefronts per workgroup = slots
#define D3P_PAIR_NONE 0xFFFFFFFFFFFFFFFFull   // the packed key of no pair: above every pair_key
#define D3P_PAIR_FORM_WIDE 1   // a workgroup per tile of a walks every tile of b
#define D3P_PAIR_FORM_SPLIT 2  // a workgroup per (tile of a, segment of b) writes cells; a second launch merges them
#define D3P_PAIR_WIDE_MIN_TILES 1024u  // the wide form is chosen where the tiles of a alone fill the chip: 256 CUs x 4 resident workgroups

namespace d3p {

// the items of a row-major table: its n rows
struct PairRows {
    typedef uint64_t index;
    const uint32_t* base; int64_t ld; uint32_t n;
    __device__ __forceinline__ bool live(uint64_t row) const { return row < n; }
    __device__ __forceinline__ uint32_t word(uint64_t row, uint32_t col) const { return base[(int64_t)row * ld + col]; }
};

__host__ __device__ __forceinline__ uint32_t pair_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + D3P_PAIR_T - 1u) / D3P_PAIR_T); }

// THE root of every walker: sqrtf, the IEEE root under the compiler's default -fhip-fp32-correctly-rounded-divide-sqrt (the
// instruction and two fma residual checks).  Not the rounded-root intrinsic: this toolchain's header hands that one to OCML's native
// root unless OCML_BASIC_ROUNDED_OPERATIONS is defined, and a device run with it lay 1 ulp off on non-square q
// (docs/experiments_fidelity.md).  d3p_pair_knn at k = 1 equals d3p_pair_stats' nearest row, and the label sums' distances are those of
// d3p_pair_stats, because this is one function
__device__ __forceinline__ float pair_sqrt(float q) { return __builtin_sqrtf(q); }

// j is a partner of row i: it exists, and it is not i itself where the diagonal is excluded
__device__ __forceinline__ bool pair_admissible(uint64_t i, uint64_t j, uint32_t nb, uint32_t excl) { return j < nb && !(excl && j == i); }

// a non-negative float's bit pattern is order-preserving: the smallest key is the smallest q, and among equal q the smallest j
__device__ __forceinline__ unsigned long long pair_key(float q, uint64_t j)
{
    return ((unsigned long long)__float_as_uint(q) << 32) | (unsigned long long)j;
}

// the 8 lanes tj = 0 .. 7 of a row under op, by the xor butterfly 4, 2, 1 in this order (op is commutative: the 8 lanes end with equal bits)
struct PairSum { template <class V> __device__ __forceinline__ V operator()(V v, V o) const { return v + o; } };
struct PairMin { template <class V> __device__ __forceinline__ V operator()(V v, V o) const { return o < v ? o : v; } };
template <class V, class OP>
__device__ __forceinline__ V pair_row_reduce(V v, OP op)
{
    for (int off = 4; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    return v;
}

// the split form's workgroups: blockIdx.x = tile of a x nseg + segment of b; a cell per (segment, row); a flag word of a's row and of b
__device__ __forceinline__ uint32_t pair_split_tile(uint32_t nseg) { return blockIdx.x / nseg; }
__device__ __forceinline__ uint32_t pair_split_segment(uint32_t nseg) { return blockIdx.x % nseg; }
__device__ __forceinline__ uint64_t pair_cell(uint32_t seg, uint32_t na, uint64_t i) { return (uint64_t)seg * na + i; }
__device__ __forceinline__ uint32_t pair_flag_word(uint32_t fa, uint32_t fb) { return fa | (fb << 1); }

__device__ __forceinline__ void pair_wave_sync()
{
    // the wavefront's own LDS: its ds operations complete in issue order; this keeps the compiler from moving them across the point
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lw: 2^lw lanes share an item of a chunk of cw <= C columns, 2^lw >= cw (at d = 2 a load instruction covers 16 items, not 2)
__device__ __forceinline__ int pair_lanes_log2(uint32_t cw) { return cw > 16 ? 5 : cw > 8 ? 4 : cw > 4 ? 3 : 2; }

// the 32 items of tile `tile` in columns c0 .. c0 + cw - 1, as raw words: lane -> (item il0 + p * (64 >> lw), column lane & (2^lw - 1));
// an item that is not live and a column beyond cw read nothing and are 0.  ITEMS: index is the type that counts its items, live(item)
// says whether the item exists, word(item, col) is its column col.  (The item is summed in this order, the pass's share last but one:
// the compiler keeps tile * T + p * (64 >> lw) in scalar registers.)
template <class ITEMS>
__device__ __forceinline__ void pair_load(const ITEMS& items, uint32_t tile, uint32_t c0, uint32_t cw, int lw, int lane, uint32_t (&w)[16])
{
    const uint32_t c = (uint32_t)lane & ((1u << lw) - 1u), il0 = (uint32_t)lane >> lw, ipp = 64u >> lw, passes = D3P_PAIR_T / ipp;
#pragma unroll
    for (uint32_t p = 0; p < 16; ++p) {
        w[p] = 0u;
        if (p < passes) {
            const typename ITEMS::index item = (typename ITEMS::index)tile * D3P_PAIR_T + il0 + p * ipp;
            if (items.live(item) && c < cw) w[p] = items.word(item, c0 + c);
        }
    }
}

// stores the chunk (dtype 1: int32 words, converted) and takes the flags of NaN and +-inf: `bad` for the whole chunk, and with rowflag a
// word per item (every lane that sets one stores 1)
__device__ __forceinline__ void pair_store(int32_t dtype, float* buf, uint32_t* rowflag, int lw, int lane, const uint32_t (&w)[16], bool& bad)
{
    const uint32_t c = (uint32_t)lane & ((1u << lw) - 1u), il0 = (uint32_t)lane >> lw, ipp = 64u >> lw, passes = D3P_PAIR_T / ipp;
#pragma unroll
    for (uint32_t p = 0; p < 16; ++p) {
        if (p < passes) {
            const float v = dtype ? (float)(int32_t)w[p] : __uint_as_float(w[p]);
            const bool nf = !(fabsf(v) <= 3.402823466e38f);   // NaN or +-inf
            bad |= nf;
            if (rowflag && nf) rowflag[il0 + p * ipp] = 1u;
            buf[(il0 + p * ipp) * D3P_PAIR_LD + c] = v;
        }
    }
}

// where d <= C a tile has one chunk, and tile I of the first side is staged once for the whole walk, by every wavefront for itself
// (with rowflag the rows' flags go there, and `bad` is the caller's to drop)
template <class ITEMS>
__device__ __forceinline__ void pair_stage_resident(const ITEMS& rows, uint32_t I, uint32_t d, int32_t dtype, float* A, uint32_t* rowflag, int lane,
                                                    bool& bad)
{
    const int lw = pair_lanes_log2(d);
    uint32_t wa[16];
    pair_load(rows, I, 0u, d, lw, lane, wa);
    pair_store(dtype, A, rowflag, lw, lane, wa, bad);
    pair_wave_sync();
}

__device__ __forceinline__ void pair_zero(float (&q)[4][4])
{
#pragma unroll
    for (int ki = 0; ki < 4; ++ki)
#pragma unroll
        for (int kj = 0; kj < 4; ++kj) q[ki][kj] = 0.0f;
}

// THE chain of one pair over four columns, ascending
__device__ __forceinline__ float pair_chain(const float4& va, const float4& vb, float q)
{
    float tt = va.x - vb.x;
    q = __fmaf_rn(tt, tt, q);
    tt = va.y - vb.y;
    q = __fmaf_rn(tt, tt, q);
    tt = va.z - vb.z;
    q = __fmaf_rn(tt, tt, q);
    tt = va.w - vb.w;
    return __fmaf_rn(tt, tt, q);
}

// ------------------------------------------------------------------------------------------------ HOST (fail and check_launch are
// d3p_host.h's, which every walker includes ahead of this file)

// THE form rule: the forced form if one is set; else the split form where the tiles of a alone cannot fill the chip and b has more
// than one segment to deal out.  The forms agree bit for bit, so the choice may look at na
inline uint32_t pair_form(int32_t forced, uint32_t tiles_a, uint32_t nseg)
{
    if (forced) return (uint32_t)forced;
    return tiles_a < D3P_PAIR_WIDE_MIN_TILES && nseg > 1u ? D3P_PAIR_FORM_SPLIT : D3P_PAIR_FORM_WIDE;
}

// the test aid behind an entry's *_set_form
inline int pair_set_form(const char* what, int32_t form, int32_t* forced)
{
    if (form != 0 && form != D3P_PAIR_FORM_WIDE && form != D3P_PAIR_FORM_SPLIT)
        return fail(D3P_E_INVALID_ARG, "%s: form must be 0 (the rule), 1 (wide) or 2 (split), got %d", what, form);
    *forced = form;
    return D3P_OK;
}

// the two launches of a form that writes cells: the walk, then the merge with one thread per row (or labelling) in groups of 256
template <class ARGS>
int pair_launch_merged(const char* what, void (*walk)(ARGS), void (*merge)(ARGS), unsigned groups, uint32_t rows, hipStream_t stream, const ARGS& a)
{
    hipLaunchKernelGGL(walk, dim3(groups), dim3(64 * D3P_PAIR_WAVES), 0, stream, a);
    const int rc = check_launch(what);
    if (rc != D3P_OK) return rc;
    hipLaunchKernelGGL(merge, dim3((unsigned)(((uint64_t)rows + 255u) / 256u)), dim3(256), 0, stream, a);
    return check_launch(what);
}

// The refusals that the entries share, in the order every entry makes them, after those of its own pointers (null, then alignment:
// each entry has its own set) and before those of its own arguments.  One table of n rows (n_name, ld_name: the entry's names for them)
inline int pair_check_table(const char* what, int32_t dtype, int64_t ld, uint32_t n, uint32_t d, const char* n_name, const char* ld_name)
{
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (n < 1) return fail(D3P_E_INVALID_ARG, "%s: %s >= 1 is required", what, n_name);
    if (d < 1) return fail(D3P_E_INVALID_ARG, "%s: d >= 1 is required", what);
    if (ld < 0 || (uint64_t)ld < d) return fail(D3P_E_INVALID_ARG, "%s: %s >= d is required", what, ld_name);
    if ((uint64_t)n > (uint64_t)INT64_MAX / (uint64_t)ld) return fail(D3P_E_INVALID_ARG, "%s: %s * %s does not fit 63 bits", what, n_name, ld_name);
    return D3P_OK;
}

// two tables a and b of one dtype and d
inline int pair_check_pair(const char* what, int32_t dtype, int64_t a_ld, int64_t b_ld, uint32_t na, uint32_t nb, uint32_t d)
{
    if (dtype != 0 && dtype != 1) return fail(D3P_E_INVALID_ARG, "%s: dtype must be 0 (float32) or 1 (int32), got %d", what, dtype);
    if (na < 1 || nb < 1) return fail(D3P_E_INVALID_ARG, "%s: na >= 1 and nb >= 1 are required", what);
    if (d < 1) return fail(D3P_E_INVALID_ARG, "%s: d >= 1 is required", what);
    if (a_ld < 0 || (uint64_t)a_ld < d) return fail(D3P_E_INVALID_ARG, "%s: a_ld >= d is required", what);
    if (b_ld < 0 || (uint64_t)b_ld < d) return fail(D3P_E_INVALID_ARG, "%s: b_ld >= d is required", what);
    if ((uint64_t)na > (uint64_t)INT64_MAX / (uint64_t)a_ld || (uint64_t)nb > (uint64_t)INT64_MAX / (uint64_t)b_ld)
        return fail(D3P_E_INVALID_ARG, "%s: na * a_ld or nb * b_ld does not fit 63 bits", what);
    return D3P_OK;
}

// the diagonal flag of a pair (d3p_pair_knn refuses its k between pair_check_pair and this: the two are not one function)
inline int pair_check_diagonal(const char* what, int32_t exclude_diagonal, uint32_t na, uint32_t nb)
{
    if (exclude_diagonal != 0 && exclude_diagonal != 1)
        return fail(D3P_E_INVALID_ARG, "%s: exclude_diagonal must be 0 or 1, got %d", what, exclude_diagonal);
    if (exclude_diagonal && na != nb)
        return fail(D3P_E_INVALID_ARG, "%s: exclude_diagonal compares a table with itself: na == nb is required (%u, %u)", what, na, nb);
    return D3P_OK;
}

}  // namespace d3p
