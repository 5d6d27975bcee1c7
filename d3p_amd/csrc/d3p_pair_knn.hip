// k nearest neighbours of two tables (d3p_amd/neighbours.py, include/d3p_hip.h): per row of the first table its k nearest
// rows of the second -- squared distance, distance and index, ascending -- and, against a squared radius per row of the second table,
// the number of those rows whose ball contains it: what improved precision and recall, density and coverage and the authenticity score
// of a synthetic table reduce.  The entry d3p_pair_knn with its host checks, its kernels, the query functions of their constants,
// forms and workspace, and the test aid that forces a form.
//
// THE RULE.  a[i * a_ld + c] is row i < na of the first table in column c < d, b[j * b_ld + c] row j < nb of the second, both float32
// (dtype 0) or both int32 (dtype 1: converted to float32 when staged, exact for |v| <= 2^24, which is what the Python layer admits).
// For a pair of rows (i, j), q(i, j) is the chain of d3p_pair_tile.h, which d3p_pair_stats.hip and d3p_energy.hip walk too:
//     t_c = fl32(a_c - b_c)      q <- fmaf(t_c, t_c, q) over c = 0 .. d-1 ascending, from q = 0
// The ADMISSIBLE j of row i are all j < nb, without j == i when exclude_diagonal is set (which requires na == nb); duplicate rows are
// pairs like any other.  A non-negative float's bit pattern is order-preserving, so the KEY of a pair is the unsigned 64-bit integer
//     (bits(q) << 32) | j
// and the keys of one row are distinct: its k smallest keys are a SET that no order of visiting changes.  For t < k, ascending:
//     q[i * k + t]     = the squared distance of the t-th smallest key
//     dist[i * k + t]  = sqrtf of it, correctly rounded (the IEEE root, pair_sqrt: not the native instruction's 1 ulp)
//     index[i * k + t] = its j           (among equal q the SMALLEST j comes first: the tie rule is on q, not on the rounded root)
// and with fewer than k admissible j the places left hold +inf, +inf, 0xFFFFFFFF.  With qr_b (nb float32 squared radii) also
//     count[i] = #{admissible j : q(i, j) < qr_b[j]}     strictly, by IEEE: a NaN radius contains nothing, +inf every finite q
// A NaN or +-inf element in row i of a makes that row's outputs NaN, NaN, 0xFFFFFFFF and its count 0xFFFFFFFF and touches no other row;
// one anywhere in b does the same to every row.  Both come from flags taken while the tables are staged, never from inf - inf.  Finite
// elements whose t_c or q overflows float32 follow IEEE from there (q = inf, ties at inf go to the smallest j like any other tie).  At
// k = 1 dist and index are d3p_pair_stats' min and argmin bit for bit: the chain, the admissible pairs, the key and the root are each
// ONE function of d3p_pair_tile.h.
//
// THE SELECTION.  The walk is d3p_pair_stats': one wavefront computes a 32 x 32 pair tile (I, J), lane l = 8 ti + tj owning the 4 x 4
// pairs (32 I + ti + 8 ki, 32 J + tj + 8 kj) in registers across chunks of C = 32 columns staged in the wavefront's own LDS (2 x 32 x
// 36 floats), and the four wavefronts of a workgroup are SLOTS that deal the tiles of b among them, J mod 4.  What is new rides on it:
//   * lane r < 32 of a slot OWNS row 32 I + r: its sorted list of the K smallest keys seen by the slot lies in 2 K of that lane's
//     registers (K = the capacity class of k: 1, 4, 8 or 16, a template parameter; the first K - k places hold the key 0, which
//     nothing sinks below, so the k smallest keys are the last k places and the threshold is place K - 1, whatever k);
//   * every lane keeps the THRESHOLD of its four rows, the row's current k-th key (all ones while the list is not full).  After a tile's
//     chain it tests its 16 keys against them -- 16 compares -- and the wavefront takes ONE ballot.  No candidate anywhere: the tile is
//     done, which is what happens to almost every tile once the lists have settled (a row expects O(k log(nb / k)) inserts in all);
//   * otherwise the tile's q is spilled to the wavefront's staging buffer of b (free after the chunk loop: the wave sync orders it),
//     the owner lanes read their row of 32 q back 16 bytes at a time, and a key below the row's threshold is inserted by a branch-free
//     chain of 64-bit min / max over the K places (lo = min(list[t], key); key = max(list[t], key)): no index into the registers, hence
//     no scratch.  The thresholds are handed back to the tile's lanes by four 64-bit shuffles;
//   * the counts are a uint32 per (lane, ki): 16 strict compares against the four radii the lane loaded for the tile; they are added
//     over tj by the xor butterfly 4, 2, 1, over the slots in LDS and over the segments in the merge (count <= nb < 2^32: no wrap);
//   * after the walk and a barrier the slots' lists are written over the staging buffers (4 x K x 32 keys <= 16 KiB of their 36 KiB),
//     and threads 0 .. 31 merge the last k places of the four lists into the row's k smallest by the same chain.
// The wide form (1) gives one workgroup one tile of a and every tile of b, and needs no workspace.  The split form (2) gives a workgroup
// one tile of a and ONE segment of G tiles of b and writes a CELL per (segment, row) -- k keys, a count and a flag word, 8 k + 8 bytes
// -- to the caller's buffer; a second launch, one thread per row, merges the cells in ascending segment order.  Every (segment, row <
// na) cell is written before it is read: the buffer's contents on entry change nothing.  The split form exists where the tiles of a
// alone cannot fill the chip; its workgroups are capped at D3P_PK_MAX_GROUPS = 4096 and G follows from the cap (a multiple of the
// slots, at least 16), so the cells take at most 4096 x 32 x (8 k + 8) bytes: 17 MiB at k = 16, whatever nb.  A table a of more than
// 4096 tiles has nothing to deal out and runs the wide form even when the split form is forced.
// Static LDS: 37904 bytes.  No atomics, no host synchronisation, no dynamic LDS, no scratch.
//
// DETERMINISM.  Everything selected is an integer minimum and everything counted an integer sum: the outputs of row i depend on that
// row's values, the table b, the radii, nb, d, k and the flag alone -- not on na, the other rows of a, a_ld, b_ld, the row's place in
// its tile, the form, the segment length (which may therefore look at na), or what the buffer held before.  The forms agree bit for
// bit and repeated calls give equal bits.
//
// Distances are NOT taken from a Gram matrix (|a|^2 + |b|^2 - 2 a.b): see d3p_pair_stats.hip and DESIGN.md 4w.
#include "d3p_device.h"
#include "d3p_host.h"
#include "d3p_pair_tile.h"

#define D3P_PK_KMAX 16               // the largest k: the largest capacity class
#define D3P_PK_MIN_G 16u             // tiles of b per segment, at least (a multiple of the slots)
#define D3P_PK_MAX_GROUPS 4096u      // workgroups of the split form, at most: bounds the workspace

static int32_t g_pk_form = 0;   // d3p_pair_knn_set_form: 0 = the rule below

namespace d3p {

typedef unsigned long long pk_key;

struct PkArgs {
    const uint32_t* a; const uint32_t* b; int32_t dtype; int64_t a_ld, b_ld; uint32_t na, nb, d, k, excl, seg_tiles, nseg;
    const float* qr; float* q; float* dist; uint32_t* index; uint32_t* count;
    pk_key* ws_key; uint32_t* ws_count; uint32_t* ws_flag;
};

// the sorted list of a row in K places: the first K - k hold the key 0, which nothing sinks below, so the row's k smallest keys lie in
// the LAST k places and the threshold is always place K - 1.  Every index is a constant after unrolling, so the list stays in registers
// (a select of place k - 1 out of the K is turned into an indexed read by the compiler, and the list into scratch).  A pair whose key
// is 0 (q = 0, j = 0) is no exception: equal values are one value to a minimum and a maximum.
template <int K>
struct PkList {
    pk_key v[K];
    __device__ __forceinline__ void clear(uint32_t k)
    {
#pragma unroll
        for (int t = 0; t < K; ++t) v[t] = (uint32_t)t < (uint32_t)K - k ? 0ull : D3P_PAIR_NONE;
    }
    // the branch-free chain: key sinks to its place, the largest of the K + 1 falls out
    __device__ __forceinline__ void insert(pk_key key)
    {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const pk_key lo = v[t] < key ? v[t] : key;
            key = v[t] < key ? key : v[t];
            v[t] = lo;
        }
    }
    // the k-th smallest key so far: the threshold
    __device__ __forceinline__ pk_key kth() const { return v[K - 1]; }
};

// the tiles J = j_lo + slot, + 4, ... < j_hi of b against tile I of a: lowers the owner lanes' lists, adds onto the lane's four counts,
// ors bad_b.  With a_resident (d <= C) tile I of a already lies in A.
template <int K>
__device__ __forceinline__ void pk_walk(const PkArgs& a, uint32_t I, uint32_t j_lo, uint32_t j_hi, uint32_t slot, float* A, float* B,
                                        uint32_t* aflag, bool a_resident, int lane, PkList<K>& list, uint32_t (&cnt)[4], bool& bad_b)
{
    const uint32_t ti = (uint32_t)lane >> 3, tj = (uint32_t)lane & 7u;
    bool bad_a = false;   // (the rows' flags go to aflag)
    const PairRows rows_a = {a.a, a.a_ld, a.na}, rows_b = {a.b, a.b_ld, a.nb};
    pk_key thr[4] = {D3P_PAIR_NONE, D3P_PAIR_NONE, D3P_PAIR_NONE, D3P_PAIR_NONE};   // of rows ti + 8 ki
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
                // the reads of the chunk before are done -- and, at a tile's first chunk, the owner lanes' float4 reads of the tile
                // spilled into B below: this sync is what orders them before the store that overwrites B
                pair_wave_sync();
                if (!a_resident) pair_store(a.dtype, A, aflag, lw, lane, wa, bad_a);
                pair_store(a.dtype, B, nullptr, lw, lane, wb, bad_b);
                pair_wave_sync();
            }
            const uint32_t cw4 = (cw + 3u) & ~3u;   // <= 2^lw: every column read below was written above
            for (uint32_t c = 0; c < cw4; c += 4) {
                float4 va[4], vb[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    va[kk] = *reinterpret_cast<const float4*>(A + (ti + 8u * kk) * D3P_PAIR_LD + c);
                    vb[kk] = *reinterpret_cast<const float4*>(B + (tj + 8u * kk) * D3P_PAIR_LD + c);
                }
#pragma unroll
                for (int ki = 0; ki < 4; ++ki)
#pragma unroll
                    for (int kj = 0; kj < 4; ++kj) q[ki][kj] = pair_chain(va[ki], vb[kj], q[ki][kj]);
            }
        }
        // the radii of the lane's four rows of b (NaN where there is none: contains nothing)
        float rad[4];
#pragma unroll
        for (int kj = 0; kj < 4; ++kj) {
            const uint64_t j = (uint64_t)J * D3P_PAIR_T + tj + 8u * kj;
            rad[kj] = a.qr && j < a.nb ? a.qr[j] : __builtin_nanf("");
        }
        bool cand = false;
#pragma unroll
        for (int ki = 0; ki < 4; ++ki) {
            const uint64_t i = (uint64_t)I * D3P_PAIR_T + ti + 8u * ki;
#pragma unroll
            for (int kj = 0; kj < 4; ++kj) {
                const uint64_t j = (uint64_t)J * D3P_PAIR_T + tj + 8u * kj;
                const bool ok = pair_admissible(i, j, a.nb, a.excl);
                cand |= ok && pair_key(q[ki][kj], j) < thr[ki];
                cnt[ki] += ok && q[ki][kj] < rad[kj] ? 1u : 0u;
            }
        }
        if (__builtin_amdgcn_ballot_w64(cand) == 0ull) continue;   // (wave-uniform)
        pair_wave_sync();   // the chunk loop's reads of B are done
#pragma unroll
        for (int ki = 0; ki < 4; ++ki)
#pragma unroll
            for (int kj = 0; kj < 4; ++kj) B[(ti + 8u * ki) * D3P_PAIR_LD + tj + 8u * kj] = q[ki][kj];
        pair_wave_sync();
        if (lane < D3P_PAIR_T) {
            const uint64_t i = (uint64_t)I * D3P_PAIR_T + (uint32_t)lane;
            for (uint32_t c = 0; c < D3P_PAIR_T; c += 4) {
                const float4 v = *reinterpret_cast<const float4*>(B + (uint32_t)lane * D3P_PAIR_LD + c);
                const float qs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint64_t j = (uint64_t)J * D3P_PAIR_T + c + (uint32_t)e;
                    const pk_key key = pair_key(qs[e], j);
                    if (pair_admissible(i, j, a.nb, a.excl) && key < list.kth()) list.insert(key);
                }
            }
        }
#pragma unroll
        for (int ki = 0; ki < 4; ++ki) thr[ki] = __shfl(list.kth(), (int)(ti + 8u * ki), 64);   // (owner lanes: < 32)
    }
}

// the outputs of row i from its k smallest keys, its count and its flags
template <int K>
__device__ __forceinline__ void pk_finish(const PkArgs& a, uint64_t i, const PkList<K>& list, uint32_t count, bool bad)
{
    const float nan = __builtin_nanf("");
    const uint32_t first = (uint32_t)K - a.k;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        if ((uint32_t)t >= first) {
            const uint64_t o = i * a.k + ((uint32_t)t - first);
            const bool none = list.v[t] == D3P_PAIR_NONE;
            const float qv = none ? __builtin_inff() : __uint_as_float((uint32_t)(list.v[t] >> 32));
            a.q[o] = bad ? nan : qv;
            a.dist[o] = bad ? nan : pair_sqrt(qv);
            a.index[o] = bad || none ? 0xFFFFFFFFu : (uint32_t)(list.v[t] & 0xFFFFFFFFull);
        }
    }
    if (a.qr) a.count[i] = bad ? 0xFFFFFFFFu : count;
}

template <int FORM, int K>
__global__ __launch_bounds__(64 * D3P_PAIR_WAVES) void k_pair_knn(PkArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[D3P_PAIR_WAVES][2][D3P_PAIR_T * D3P_PAIR_LD];
    __shared__ uint32_t slot_count[D3P_PAIR_WAVES][D3P_PAIR_T];
    __shared__ uint32_t slot_aflag[D3P_PAIR_WAVES][D3P_PAIR_T];
    __shared__ uint32_t slot_bflag[D3P_PAIR_WAVES];
    static_assert(sizeof(pk_key) * D3P_PAIR_WAVES * K * D3P_PAIR_T <= sizeof(lds), "the slots' lists lie over the staging buffers");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ti = (uint32_t)lane >> 3, tj = (uint32_t)lane & 7u;
    float* A = lds[wave][0];
    float* B = lds[wave][1];
    uint32_t* aflag = slot_aflag[wave];
    const uint32_t ntb = pair_tiles(a.nb);
    const uint32_t I = FORM == D3P_PAIR_FORM_WIDE ? blockIdx.x : pair_split_tile(a.nseg);
    const uint32_t seg = FORM == D3P_PAIR_FORM_WIDE ? 0u : pair_split_segment(a.nseg);
    const uint32_t j_lo = FORM == D3P_PAIR_FORM_WIDE ? 0u : seg * a.seg_tiles;                       // nseg * seg_tiles < ntb + seg_tiles: no wrap
    const uint32_t j_hi = FORM == D3P_PAIR_FORM_WIDE || ntb - j_lo < a.seg_tiles ? ntb : j_lo + a.seg_tiles;
    if (lane < D3P_PAIR_T) aflag[lane] = 0u;
    pair_wave_sync();
    const bool a_resident = a.d <= D3P_PAIR_C;
    bool bad_b = false;
    if (a_resident) {
        bool bad_a = false;
        pair_stage_resident(PairRows{a.a, a.a_ld, a.na}, I, a.d, a.dtype, A, aflag, lane, bad_a);
    }
    PkList<K> list;
    list.clear(a.k);
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};
    pk_walk<K>(a, I, j_lo, j_hi, (uint32_t)wave, A, B, aflag, a_resident, lane, list, cnt, bad_b);
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
        const uint32_t c = pair_row_reduce(cnt[ki], PairSum());
        if (tj == 0) slot_count[wave][ti + 8u * ki] = c;
    }
    bad_b = __builtin_amdgcn_ballot_w64(bad_b) != 0ull;
    if (lane == 0) slot_bflag[wave] = bad_b ? 1u : 0u;
    __syncthreads();   // every slot is done with its staging buffers: the lists go over them
    pk_key* slot_list = reinterpret_cast<pk_key*>(&lds[0][0][0]);   // [slot][place][row]
    if (lane < D3P_PAIR_T) {
#pragma unroll
        for (int t = 0; t < K; ++t) slot_list[((uint32_t)wave * K + t) * D3P_PAIR_T + lane] = list.v[t];
    }
    __syncthreads();
    if (threadIdx.x < D3P_PAIR_T) {
        const uint64_t i = (uint64_t)I * D3P_PAIR_T + threadIdx.x;
        if (i < a.na) {
            PkList<K> all;
            all.clear(a.k);
            uint32_t count = 0u, fa = 0u, fb = 0u;
            for (uint32_t w = 0; w < D3P_PAIR_WAVES; ++w) {
                for (uint32_t t = (uint32_t)K - a.k; t < (uint32_t)K; ++t) all.insert(slot_list[(w * K + t) * D3P_PAIR_T + threadIdx.x]);
                count += slot_count[w][threadIdx.x];
                fa |= slot_aflag[w][threadIdx.x];
                fb |= slot_bflag[w];
            }
            if (FORM == D3P_PAIR_FORM_WIDE) {
                pk_finish<K>(a, i, all, count, (fa | fb) != 0u);
            } else {
                const uint64_t cell = pair_cell(seg, a.na, i);
#pragma unroll
                for (int t = 0; t < K; ++t)
                    if ((uint32_t)t >= (uint32_t)K - a.k) a.ws_key[cell * a.k + ((uint32_t)t - ((uint32_t)K - a.k))] = all.v[t];
                a.ws_count[cell] = count;
                a.ws_flag[cell] = pair_flag_word(fa, fb);
            }
        }
    }
}

// the split form's second launch: one thread per row merges its cells in ascending segment order
template <int K>
__global__ __launch_bounds__(256) void k_pair_knn_merge(PkArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.na) return;
    PkList<K> all;
    all.clear(a.k);
    uint32_t count = 0u, flags = 0u;
    for (uint32_t seg = 0; seg < a.nseg; ++seg) {
        const uint64_t cell = pair_cell(seg, a.na, i);
        for (uint32_t t = 0; t < a.k; ++t) {
            const pk_key key = a.ws_key[cell * a.k + t];
            if (key < all.kth()) all.insert(key);
        }
        count += a.ws_count[cell];
        flags |= a.ws_flag[cell];
    }
    pk_finish<K>(a, i, all, count, flags != 0u);
}

static uint32_t pk_capacity(uint32_t k) { return k <= 1u ? 1u : k <= 4u ? 4u : k <= 8u ? 8u : 16u; }

static bool pk_admissible(uint32_t na, uint32_t nb, uint32_t d, uint32_t k) { return na >= 1 && nb >= 1 && d >= 1 && k >= 1 && k <= D3P_PK_KMAX; }

// tiles of b per segment of the split form: at most D3P_PK_MAX_GROUPS workgroups in all, a multiple of the slots, at least D3P_PK_MIN_G
static uint32_t pk_segment_tiles(uint32_t na, uint32_t nb)
{
    const uint32_t ta = pair_tiles(na), tb = pair_tiles(nb);
    const uint32_t most = ta >= D3P_PK_MAX_GROUPS ? 1u : D3P_PK_MAX_GROUPS / ta;   // segments, at most
    uint32_t g = (tb + most - 1u) / most;                                          // <= 2^27
    g = (g + D3P_PAIR_WAVES - 1u) / D3P_PAIR_WAVES * D3P_PAIR_WAVES;
    return g < D3P_PK_MIN_G ? D3P_PK_MIN_G : g;
}

static uint32_t pk_segments(uint32_t na, uint32_t nb)
{
    const uint32_t g = pk_segment_tiles(na, nb);
    return (pair_tiles(nb) + g - 1u) / g;
}

static uint32_t pk_form(uint32_t na, uint32_t nb, uint32_t d, uint32_t k)
{
    if (!pk_admissible(na, nb, d, k)) return 0;
    if (pair_tiles(na) > D3P_PK_MAX_GROUPS) return D3P_PAIR_FORM_WIDE;   // nothing to deal out, and the cells would not be bounded
    return pair_form(g_pk_form, pair_tiles(na), pk_segments(na, nb));
}

static size_t pk_workspace(uint32_t na, uint32_t nb, uint32_t d, uint32_t k)
{
    if (pk_form(na, nb, d, k) != D3P_PAIR_FORM_SPLIT) return 0;
    return (size_t)pk_segments(na, nb) * (size_t)na * (8u * (size_t)k + 8u);   // <= 4096 x 32 x 136
}

template <int K>
static int pk_launch(const char* what, uint32_t form, unsigned groups, hipStream_t stream, const PkArgs& a)
{
    if (form == D3P_PAIR_FORM_WIDE) {
        hipLaunchKernelGGL((k_pair_knn<D3P_PAIR_FORM_WIDE, K>), dim3(groups), dim3(64 * D3P_PAIR_WAVES), 0, stream, a);
        return check_launch(what);
    }
    return pair_launch_merged(what, k_pair_knn<D3P_PAIR_FORM_SPLIT, K>, k_pair_knn_merge<K>, groups, a.na, stream, a);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_pair_knn_max_k(void) { return D3P_PK_KMAX; }

uint32_t d3p_pair_knn_tile_rows(void) { return D3P_PAIR_T; }

uint32_t d3p_pair_knn_chunk_cols(void) { return D3P_PAIR_C; }

uint32_t d3p_pair_knn_capacity(uint32_t k) { return k >= 1 && k <= D3P_PK_KMAX ? pk_capacity(k) : 0u; }

uint32_t d3p_pair_knn_form(uint32_t na, uint32_t nb, uint32_t d, uint32_t k) { return pk_form(na, nb, d, k); }

size_t d3p_pair_knn_workspace(uint32_t na, uint32_t nb, uint32_t d, uint32_t k) { return pk_workspace(na, nb, d, k); }

uint32_t d3p_pair_knn_segment_tiles(uint32_t na, uint32_t nb, uint32_t d, uint32_t k)
{
    return pk_admissible(na, nb, d, k) ? pk_segment_tiles(na, nb) : 0u;
}

int d3p_pair_knn_set_form(int32_t form) { return pair_set_form("d3p_pair_knn_set_form", form, &g_pk_form); }

int d3p_pair_knn(void* stream, const void* a_dev, const void* b_dev, int32_t dtype, int64_t a_ld, int64_t b_ld, uint32_t na, uint32_t nb,
                 uint32_t d, uint32_t k, int32_t exclude_diagonal, const float* qr_b_dev, float* q_dev, float* dist_dev, uint32_t* index_dev,
                 uint32_t* count_dev, void* ws_dev, size_t ws_bytes)
{
    const char* what = "d3p_pair_knn";
    if (!a_dev || !b_dev || !q_dev || !dist_dev || !index_dev || (qr_b_dev && !count_dev)) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)a_dev | (uintptr_t)b_dev | (uintptr_t)qr_b_dev | (uintptr_t)q_dev | (uintptr_t)dist_dev | (uintptr_t)index_dev |
          (uintptr_t)count_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if (((uintptr_t)ws_dev & 7u) != 0) return fail(D3P_E_INVALID_ARG, "%s: ws_dev is not aligned to 8 bytes", what);
    if (const int rc = pair_check_pair(what, dtype, a_ld, b_ld, na, nb, d)) return rc;
    if (k < 1 || k > D3P_PK_KMAX) return fail(D3P_E_INVALID_ARG, "%s: 1 <= k <= %d is required, got %u", what, D3P_PK_KMAX, k);
    if (const int rc = pair_check_diagonal(what, exclude_diagonal, na, nb)) return rc;
    const uint32_t form = pk_form(na, nb, d, k);
    const size_t need = pk_workspace(na, nb, d, k);
    if (ws_bytes < need || (need && !ws_dev))
        return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_dev ? ws_bytes : (size_t)0, need);
    const uint32_t nseg = pk_segments(na, nb);
    // one workgroup per tile of a (< 2^27) or, split, per tile and segment (<= D3P_PK_MAX_GROUPS + the tiles of a): no grid to refuse
    const uint64_t groups = (uint64_t)pair_tiles(na) * (form == D3P_PAIR_FORM_SPLIT ? nseg : 1u);
    if (!is_device_ptr(a_dev) || !is_device_ptr(b_dev) || !is_device_ptr(q_dev) || !is_device_ptr(dist_dev) || !is_device_ptr(index_dev) ||
        (qr_b_dev && (!is_device_ptr(qr_b_dev) || !is_device_ptr(count_dev))) || (need && !is_device_ptr(ws_dev)))
        return fail(D3P_E_INVALID_ARG, "%s: the tables, the radii, the outputs and the workspace must be device memory", what);
    PkArgs a;
    a.a = static_cast<const uint32_t*>(a_dev); a.b = static_cast<const uint32_t*>(b_dev); a.dtype = dtype; a.a_ld = a_ld; a.b_ld = b_ld;
    a.na = na; a.nb = nb; a.d = d; a.k = k; a.excl = (uint32_t)exclude_diagonal; a.seg_tiles = pk_segment_tiles(na, nb); a.nseg = nseg;
    a.qr = qr_b_dev; a.q = q_dev; a.dist = dist_dev; a.index = index_dev; a.count = count_dev;
    const size_t cells = (size_t)nseg * na;
    a.ws_key = static_cast<pk_key*>(ws_dev);
    a.ws_count = need ? reinterpret_cast<uint32_t*>(static_cast<char*>(ws_dev) + 8u * (size_t)k * cells) : nullptr;
    a.ws_flag = need ? a.ws_count + cells : nullptr;
    switch (pk_capacity(k)) {
    case 1: return pk_launch<1>(what, form, (unsigned)groups, (hipStream_t)stream, a);
    case 4: return pk_launch<4>(what, form, (unsigned)groups, (hipStream_t)stream, a);
    case 8: return pk_launch<8>(what, form, (unsigned)groups, (hipStream_t)stream, a);
    default: return pk_launch<16>(what, form, (unsigned)groups, (hipStream_t)stream, a);
    }
}

}  // extern "C"
