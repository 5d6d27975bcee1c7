// The wavefront-private 32 x 32 tile of squared distances that the energy score (d3p_energy.hip) and the pair statistics
// (d3p_pair_stats.hip) walk, one definition each: the tile's constants, the wave sync of its LDS, the lane -> (item,
// column) map of a staged chunk with its load and store, and the chain
//     t_c = fl32(a_c - b_c)      q <- fmaf(t_c, t_c, q)      over c ascending
// of one pair over four columns.  A wavefront stages C = 32 columns of the 32 items of each side in its own 2 x 32 x 36 floats of LDS
// (load -> wave sync -> store -> wave sync); lane 8 ti + tj keeps the 4 x 4 pairs (ti + 8 ki, tj + 8 kj) in registers across the chunks
// and reads its 4 + 4 rows 16 bytes at a time.  What the items are, the walk over tiles, slots and segments, the column loop over a
// chunk (a dozen lines: as a helper it cost a wave of occupancy, docs/experiments_fidelity.md), the root and the epilogues stay their
// files' own.
#pragma once
#include "d3p_device.h"

#define D3P_PAIR_T 32          // items per side of a pair tile
#define D3P_PAIR_C 32          // columns per staged chunk
#define D3P_PAIR_LD 36         // LDS row stride in floats (a multiple of 4: the reads are 16 bytes wide)
#define D3P_PAIR_WAVES 4       // wavefronts per workgroup = slots

namespace d3p {

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

}  // namespace d3p
