// Mixed-type (Gower) pair statistics of two tables (d3p_amd/mixed.py, include/d3p_hip.h): d3p_pair_stats' three outputs per
// row of the first table -- the float64 sum of its distances to the rows of the second, the distance to its nearest row there and that
// row's index -- under a distance that serves tables whose columns are partly category codes: a weighted L1 sum over the numeric columns
// plus a weighted count of the categorical columns whose codes differ.  The entry d3p_pair_stats_mixed with its host checks, the schema
// and pack launches, the walker of the PACKED tables, the query functions and the test aid that forces a form.
//
// THE SCHEMA.  kind[c] (uint8: 0 numeric, 1 categorical) and scale[c] (float32, finite and >= 0, read for numeric columns only: the
// Python layer passes weight_c / range_c, rounded once from float64, and 0 for a constant column) are HOST arrays of d elements, which
// the entry checks and copies to the device as launch arguments (256 packed positions a launch: no copy call, no host synchronisation);
// w_cat >= 0 is the one weight of a categorical mismatch.  dn is the number of numeric columns, dc of categorical ones, d = dn + dc >= 1
// in any split.
//
// THE PACK (k_mixed_pack, once per table).  Row i of a row-major float32 (dtype 0) or int32 (dtype 1: converted to float32, exact for
// |v| <= 2^24) table becomes a row of d3p_pair_mixed_packed_words(dn, dc) = 4 ceil(dn / 4) + ceil(dc / 4) words:
//   * the numeric columns first, in ascending c, as floats u = fl32(x_c * scale_c), zero-padded to a multiple of 4 words;
//   * the categorical columns after them, in ascending c, as byte codes four to a word, the lowest byte first, pad bytes 0.
// A row's flag word is 1 when a numeric value or its product is NaN or +-inf, or a categorical value is not an integer in [0, 255]
// (float32: v == truncf(v) and in range; -0 is the code 0), else 0.  2^lw >= min(d + pads, 64) lanes share a row and read it along the
// row: one coalesced pass over each table.
//
// THE RULE.  For a pair of packed rows (i, j):
//     qn = the float32 chain qn <- qn + |fl32(u_ik - u_jk)| over the numeric words k ascending, from +0   (a subtract and an add of its
//          absolute value: two roundings a column, nothing to contract)
//     m  = the number of categorical columns whose codes differ, an exact integer
//     dist = fmaf(w_cat, (float)m, qn), one rounding.  No root.  Zero padding adds +0 to qn and never a mismatch.
// The ADMISSIBLE j, sum[i], min[i], argmin[i], the row without an admissible j and the flagged rows are d3p_pair_stats': the float64
// sum of (double)dist, the smallest dist, the SMALLEST j attaining it through ONE unsigned 64-bit minimum of pair_key(dist, j) =
// (bits(dist) << 32) | j; 0, +inf, 0xFFFFFFFF with no admissible j; NaN, NaN, 0xFFFFFFFF for a flagged row of a alone and, with a flagged
// row anywhere in b, for every row.  The flags are the pack's, never inf - inf; finite values whose difference or sum overflows follow
// IEEE (dist = inf, ties at inf to the smallest j).
//
// THE ORDER of the float64 sum of row i is d3p_pair_stats.hip's, word for word: tiles of T = 32 rows of b, segments of G = 16 tiles
// (d3p_pair_stats_mixed_segment_tiles), tile J in slot J mod 4; lane 8 ti + tj of a wavefront owns the pairs (ti + 8 ki, tj + 8 kj) and
// adds, per ki, its dist in the order kj = 0 .. 3 onto ONE float64 sum over the slot's tiles in ascending J; the 8 lanes of a row meet by
// the xor butterfly 4, 2, 1; per segment the four slot sums are added in ascending order onto 0, and the segments in ascending segment
// order onto 0.  The wide form (1) and the split form (2: cells of a float64 sum, a packed minimum and a flag word per (segment, row),
// and a merge launch) walk that one order: the forms agree bit for bit.
//
// THE WALKER (k_pair_mixed<FORM>) stages RAW WORDS of the packed tables, 32 words a chunk, in its wavefront's own LDS (2 x 32 x 36 words):
// no conversion and no flag scan while staging.  Every 16-byte LDS read is wholly numeric or wholly categorical: the branch is on the
// word offset against 4 ceil(dn / 4) and is wave-uniform.  A numeric group runs the chain above; a categorical group takes a ^ b per
// word, marks its non-zero bytes without a carry between them (((x & 0x7f7f7f7f) + 0x7f7f7f7f) | x) & 0x80808080, and a population
// count adds them onto the pair's uint32 count, which stays in registers across the chunks beside qn.  The tile of a is resident where
// the packed row fits one chunk (up to 128 categorical columns, or 16 numeric + 64 categorical).  Static LDS: 39952 bytes.  No atomics,
// no scratch, no dynamic LDS, no host synchronisation or allocation.
//
// THE WORKSPACE (d3p_pair_stats_mixed_workspace(na, nb, dn, dc) bytes) holds, in this order: the split form's cells (20 bytes per
// (segment, row)), the packed positions (2 words each), the packed tables of a and b, and their row flags.  Every word read is written
// earlier in the same call: what it held on entry changes nothing.
//
// DETERMINISM.  Repeated calls give equal bits.  The three outputs of row i depend on that row's values, the table b, nb, the schema and
// the flag alone: not on na, the other rows of a, a_ld, b_ld, the row's place in its tile, the form, or what the workspace held before.
#include "d3p_device.h"
#include "d3p_host.h"
#include "d3p_pair_tile.h"

#define D3P_PM_G 16          // tiles of b per segment (a multiple of the slots)
#define D3P_PM_CELL 20u      // bytes per (segment, row) of the split form: a double, a packed minimum, a flag word
#define D3P_PM_SLOTS 256u    // packed positions that one schema launch carries in its arguments
#define D3P_PM_MAX_D (1u << 28)   // a position is 30 bits of a word: byte offsets of up to 2^28 codes and their padding fit

static int32_t g_pm_form = 0;   // d3p_pair_stats_mixed_set_form: 0 = the rule below

namespace d3p {

// a packed position: w[0] = what << 30 | where, w[1] = the bits of scale.  what 0: numeric column s -> word `where`; 1: categorical
// column s -> byte `where` of the categorical words; 2: a zero word at `where`; 3: a zero byte at `where`.  Positions 0 .. d-1 are the
// columns, the padding follows them
struct MxSlots { uint32_t w[2 * D3P_PM_SLOTS]; uint32_t base, count; uint32_t* slot; };

__global__ __launch_bounds__(D3P_PM_SLOTS) void k_mixed_schema(MxSlots s)
{
    if (threadIdx.x < s.count) {
        s.slot[2u * (s.base + threadIdx.x)] = s.w[2u * threadIdx.x];
        s.slot[2u * (s.base + threadIdx.x) + 1u] = s.w[2u * threadIdx.x + 1u];
    }
}

struct MxPackArgs {
    const uint32_t* x; int64_t ld; uint32_t n, d, ns, pw, dn4; int32_t dtype; int32_t lw;
    const uint32_t* slot; uint32_t* packed; uint32_t* flag;
};

// 2^lw lanes share a row: lane -> (row, position s = sub, sub + 2^lw, ..); every position of a live row is written, and its flag word
__global__ __launch_bounds__(256) void k_mixed_pack(MxPackArgs p)
{
    const uint32_t g = 1u << p.lw, sub = threadIdx.x & (g - 1u);
    const uint64_t row = (uint64_t)blockIdx.x * (256u >> p.lw) + (threadIdx.x >> p.lw);
    const bool live = row < p.n;
    bool bad = false;
    if (live) {
        const uint32_t* src = p.x + (int64_t)row * p.ld;
        uint32_t* prow = p.packed + row * p.pw;
        float* nums = reinterpret_cast<float*>(prow);
        uint8_t* codes = reinterpret_cast<uint8_t*>(prow + p.dn4);
        for (uint32_t s = sub; s < p.ns; s += g) {
            const uint32_t meta = p.slot[2u * s], what = meta >> 30, where = meta & 0x3FFFFFFFu;
            float v = 0.0f;
            if (s < p.d) v = p.dtype ? (float)(int32_t)src[s] : __uint_as_float(src[s]);
            if (what == 0u) {
                const float u = v * __uint_as_float(p.slot[2u * s + 1u]);
                bad |= !(fabsf(v) <= 3.402823466e38f) || !(fabsf(u) <= 3.402823466e38f);   // NaN or +-inf
                nums[where] = u;
            } else if (what == 1u) {
                const bool ok = v == truncf(v) && v >= 0.0f && v <= 255.0f;   // (NaN fails the first)
                bad |= !ok;
                codes[where] = ok ? (uint8_t)(uint32_t)v : (uint8_t)0;
            } else if (what == 2u) {
                prow[where] = 0u;
            } else {
                codes[where] = (uint8_t)0;
            }
        }
    }
    const unsigned long long any = __builtin_amdgcn_ballot_w64(bad);
    const uint32_t first = (threadIdx.x & 63u) & ~(g - 1u);   // the row's lanes of this wavefront: first .. first + g - 1
    const unsigned long long mine = g == 64u ? ~0ull : ((1ull << g) - 1ull) << first;
    if (live && sub == 0u) p.flag[row] = (any & mine) != 0ull ? 1u : 0u;
}

struct MxArgs {
    const uint32_t* a; const uint32_t* b; const uint32_t* aflag; const uint32_t* bflag;
    uint32_t na, nb, pw, dn4, excl, nseg; float w_cat;
    double* sum; float* min; uint32_t* argmin;
    double* ws_sum; unsigned long long* ws_min; uint32_t* ws_flag;
};

// stores a loaded chunk as it is: raw words
__device__ __forceinline__ void mx_store(uint32_t* buf, int lw, int lane, const uint32_t (&w)[16])
{
    const uint32_t c = (uint32_t)lane & ((1u << lw) - 1u), il0 = (uint32_t)lane >> lw, ipp = 64u >> lw, passes = D3P_PAIR_T / ipp;
#pragma unroll
    for (uint32_t p = 0; p < 16; ++p)
        if (p < passes) buf[(il0 + p * ipp) * D3P_PAIR_LD + c] = w[p];
}

// THE numeric chain of one pair over four words, ascending
__device__ __forceinline__ float mx_chain(const uint4& va, const uint4& vb, float q)
{
    q = q + fabsf(__uint_as_float(va.x) - __uint_as_float(vb.x));
    q = q + fabsf(__uint_as_float(va.y) - __uint_as_float(vb.y));
    q = q + fabsf(__uint_as_float(va.z) - __uint_as_float(vb.z));
    return q + fabsf(__uint_as_float(va.w) - __uint_as_float(vb.w));
}

// the non-zero bytes of x, counted onto m: bit 7 of a byte is set where its low seven bits carry into it or it is set already
__device__ __forceinline__ uint32_t mx_differ(uint32_t x, uint32_t m)
{
    return m + (uint32_t)__builtin_popcount((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
}

__device__ __forceinline__ uint32_t mx_count(const uint4& va, const uint4& vb, uint32_t m)
{
    m = mx_differ(va.x ^ vb.x, m);
    m = mx_differ(va.y ^ vb.y, m);
    m = mx_differ(va.z ^ vb.z, m);
    return mx_differ(va.w ^ vb.w, m);
}

// the tiles of one slot of one segment against tile I of a: adds onto the lane's four sums, lowers its four packed minima, ors the
// flags of the rows of b it meets.  With a_resident (pw <= C) tile I of a already lies in A.
__device__ __forceinline__ void mx_segment_slot(const MxArgs& a, uint32_t I, uint32_t seg, uint32_t slot, uint32_t* A, uint32_t* B, bool a_resident,
                                                int lane, double (&ls)[4], unsigned long long (&pm)[4], bool& bad_b)
{
    const uint32_t ntb = pair_tiles(a.nb);
    const uint32_t j_lo = seg * D3P_PM_G, j_hi = ntb - j_lo < D3P_PM_G ? ntb : j_lo + D3P_PM_G;
    const uint32_t ti = (uint32_t)lane >> 3, tj = (uint32_t)lane & 7u;
    const PairRows rows_a = {a.a, (int64_t)a.pw, a.na}, rows_b = {a.b, (int64_t)a.pw, a.nb};
    for (uint32_t J = j_lo + slot; J < j_hi; J += D3P_PAIR_WAVES) {
        const uint64_t jf = (uint64_t)J * D3P_PAIR_T + (uint32_t)lane;
        if (lane < D3P_PAIR_T && jf < a.nb) bad_b |= a.bflag[jf] != 0u;
        float q[4][4];
        uint32_t m[4][4];
        pair_zero(q);
#pragma unroll
        for (int ki = 0; ki < 4; ++ki)
#pragma unroll
            for (int kj = 0; kj < 4; ++kj) m[ki][kj] = 0u;
        for (uint32_t c0 = 0; c0 < a.pw; c0 += D3P_PAIR_C) {
            const uint32_t cw = a.pw - c0 < D3P_PAIR_C ? a.pw - c0 : D3P_PAIR_C;
            const int lw = pair_lanes_log2(cw);
            {
                uint32_t wa[16], wb[16];
                if (!a_resident) pair_load(rows_a, I, c0, cw, lw, lane, wa);
                pair_load(rows_b, J, c0, cw, lw, lane, wb);
                pair_wave_sync();   // the reads of the chunk before are done
                if (!a_resident) mx_store(A, lw, lane, wa);
                mx_store(B, lw, lane, wb);
                pair_wave_sync();
            }
            const uint32_t cw4 = (cw + 3u) & ~3u;   // <= 2^lw: every word read below was written above
            for (uint32_t c = 0; c < cw4; c += 4) {
                uint4 va[4], vb[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    va[k] = *reinterpret_cast<const uint4*>(A + (ti + 8u * k) * D3P_PAIR_LD + c);
                    vb[k] = *reinterpret_cast<const uint4*>(B + (tj + 8u * k) * D3P_PAIR_LD + c);
                }
                if (c0 + c < a.dn4) {   // (wave-uniform: dn4 is a multiple of 4, and so is every c0 + c)
#pragma unroll
                    for (int ki = 0; ki < 4; ++ki)
#pragma unroll
                        for (int kj = 0; kj < 4; ++kj) q[ki][kj] = mx_chain(va[ki], vb[kj], q[ki][kj]);
                } else {
#pragma unroll
                    for (int ki = 0; ki < 4; ++ki)
#pragma unroll
                        for (int kj = 0; kj < 4; ++kj) m[ki][kj] = mx_count(va[ki], vb[kj], m[ki][kj]);
                }
            }
        }
#pragma unroll
        for (int ki = 0; ki < 4; ++ki) {
            const uint64_t i = (uint64_t)I * D3P_PAIR_T + ti + 8u * ki;
#pragma unroll
            for (int kj = 0; kj < 4; ++kj) {
                const uint64_t j = (uint64_t)J * D3P_PAIR_T + tj + 8u * kj;
                const bool ok = pair_admissible(i, j, a.nb, a.excl);
                const float dist = __fmaf_rn(a.w_cat, (float)m[ki][kj], q[ki][kj]);
                ls[ki] += ok ? (double)dist : 0.0;
                const unsigned long long key = pair_key(dist, j);
                pm[ki] = ok && key < pm[ki] ? key : pm[ki];
            }
        }
    }
}

// the three outputs of row i from its float64 sum, its packed minimum and its flags
__device__ __forceinline__ void mx_finish(const MxArgs& a, uint64_t i, double total, unsigned long long key, bool bad)
{
    const float nan = __builtin_nanf("");
    const bool none = key == D3P_PAIR_NONE;
    a.sum[i] = bad ? (double)nan : total;
    a.min[i] = bad ? nan : none ? __builtin_inff() : __uint_as_float((uint32_t)(key >> 32));
    a.argmin[i] = bad || none ? 0xFFFFFFFFu : (uint32_t)(key & 0xFFFFFFFFull);
}

template <int FORM>
__global__ __launch_bounds__(64 * D3P_PAIR_WAVES) void k_pair_mixed(MxArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[D3P_PAIR_WAVES][2][D3P_PAIR_T * D3P_PAIR_LD];
    __shared__ double slot_sum[2][D3P_PAIR_WAVES][D3P_PAIR_T];
    __shared__ unsigned long long slot_min[D3P_PAIR_WAVES][D3P_PAIR_T];
    __shared__ uint32_t slot_bflag[D3P_PAIR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ti = (uint32_t)lane >> 3, tj = (uint32_t)lane & 7u;
    uint32_t* A = lds[wave][0];
    uint32_t* B = lds[wave][1];
    const uint32_t I = FORM == D3P_PAIR_FORM_WIDE ? blockIdx.x : pair_split_tile(a.nseg);
    const uint32_t seg_lo = FORM == D3P_PAIR_FORM_WIDE ? 0u : pair_split_segment(a.nseg);
    const uint32_t seg_hi = FORM == D3P_PAIR_FORM_WIDE ? a.nseg : seg_lo + 1u;
    const bool a_resident = a.pw <= D3P_PAIR_C;
    if (a_resident) {   // one chunk: tile I of a is staged once for the whole walk, by every wavefront for itself
        const int lw = pair_lanes_log2(a.pw);
        uint32_t wa[16];
        pair_load(PairRows{a.a, (int64_t)a.pw, a.na}, I, 0u, a.pw, lw, lane, wa);
        mx_store(A, lw, lane, wa);
        pair_wave_sync();
    }
    bool bad_b = false;
    unsigned long long pm[4] = {D3P_PAIR_NONE, D3P_PAIR_NONE, D3P_PAIR_NONE, D3P_PAIR_NONE};
    double total = 0.0;   // (threads 0 .. 31: row 32 I + threadIdx.x)
    for (uint32_t seg = seg_lo; seg < seg_hi; ++seg) {
        double ls[4] = {0.0, 0.0, 0.0, 0.0};
        mx_segment_slot(a, I, seg, (uint32_t)wave, A, B, a_resident, lane, ls, pm, bad_b);
        const uint32_t par = seg & 1u;
#pragma unroll
        for (int ki = 0; ki < 4; ++ki) {
            const double s = pair_row_reduce(ls[ki], PairSum());
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
        const unsigned long long m = pair_row_reduce(pm[ki], PairMin());
        if (tj == 0) slot_min[wave][ti + 8u * ki] = m;
    }
    bad_b = __builtin_amdgcn_ballot_w64(bad_b) != 0ull;
    if (lane == 0) slot_bflag[wave] = bad_b ? 1u : 0u;
    __syncthreads();
    if (threadIdx.x < D3P_PAIR_T) {
        const uint64_t i = (uint64_t)I * D3P_PAIR_T + threadIdx.x;
        if (i < a.na) {
            unsigned long long key = D3P_PAIR_NONE;
            uint32_t fb = 0u;
            const uint32_t fa = a.aflag[i];
            for (int w = 0; w < D3P_PAIR_WAVES; ++w) {
                key = slot_min[w][threadIdx.x] < key ? slot_min[w][threadIdx.x] : key;
                fb |= slot_bflag[w];
            }
            if (FORM == D3P_PAIR_FORM_WIDE) {
                mx_finish(a, i, total, key, (fa | fb) != 0u);
            } else {
                const uint64_t cell = pair_cell(seg_lo, a.na, i);
                a.ws_sum[cell] = total;
                a.ws_min[cell] = key;
                a.ws_flag[cell] = pair_flag_word(fa, fb);
            }
        }
    }
}

// the split form's second launch: one thread per row adds its cells in ascending segment order
__global__ __launch_bounds__(256) void k_pair_mixed_merge(MxArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.na) return;
    double total = 0.0;
    unsigned long long key = D3P_PAIR_NONE;
    uint32_t flags = 0u;
    for (uint32_t seg = 0; seg < a.nseg; ++seg) {
        const uint64_t cell = pair_cell(seg, a.na, i);
        total += a.ws_sum[cell];
        key = a.ws_min[cell] < key ? a.ws_min[cell] : key;
        flags |= a.ws_flag[cell];
    }
    mx_finish(a, i, total, key, flags != 0u);
}

static uint32_t mx_segments(uint32_t nb) { return (pair_tiles(nb) + D3P_PM_G - 1u) / D3P_PM_G; }

static uint32_t mx_form(uint32_t na, uint32_t nb, uint32_t d)
{
    if (na < 1 || nb < 1 || d < 1) return 0;
    return pair_form(g_pm_form, pair_tiles(na), mx_segments(nb));
}

static uint32_t mx_num_words(uint32_t dn) { return (uint32_t)(((uint64_t)dn + 3u) & ~3ull); }

static uint64_t mx_packed_words(uint32_t dn, uint32_t dc) { return (uint64_t)mx_num_words(dn) + ((uint64_t)dc + 3u) / 4u; }

// the packed positions: the d columns, the zero words after the numeric ones and the zero bytes after the codes
static uint64_t mx_positions(uint32_t dn, uint32_t dc) { return (uint64_t)dn + dc + (mx_num_words(dn) - dn) + ((4u - (dc & 3u)) & 3u); }

struct MxLayout { size_t cells, slot, pa, pb, fa, fb, total; };

static MxLayout mx_layout(uint32_t na, uint32_t nb, uint32_t dn, uint32_t dc)
{
    MxLayout l = {};
    const uint64_t d = (uint64_t)dn + dc;
    if (na < 1 || nb < 1 || d < 1 || d > D3P_PM_MAX_D) return l;
    const size_t pw = (size_t)mx_packed_words(dn, dc);
    l.cells = mx_form(na, nb, (uint32_t)d) == D3P_PAIR_FORM_SPLIT ? (size_t)mx_segments(nb) * na * D3P_PM_CELL : 0;   // < 2^23 x 2^32 x 20
    l.slot = l.cells;
    l.pa = l.slot + 8u * (size_t)mx_positions(dn, dc);
    l.pb = l.pa + 4u * pw * na;          // < 2^2 x 2^28 x 2^32: no wrap
    l.fa = l.pb + 4u * pw * nb;
    l.fb = l.fa + 4u * (size_t)na;
    l.total = l.fb + 4u * (size_t)nb;
    return l;
}

// the schema's launches: the positions in order, D3P_PM_SLOTS a launch, built in the launch's own arguments
static int mx_upload_schema(const char* what, hipStream_t stream, const uint8_t* kind, const float* scale, uint32_t d, uint32_t dn, uint32_t dc,
                            uint32_t* slot_dev)
{
    MxSlots s;
    s.slot = slot_dev;
    s.base = 0u;
    s.count = 0u;
    const uint32_t ns = (uint32_t)mx_positions(dn, dc), dn4 = mx_num_words(dn);
    uint32_t num = 0u, cat = 0u;
    for (uint32_t p = 0; p < ns; ++p) {
        uint32_t what_p, where;
        float sc = 0.0f;
        if (p < d && kind[p] == 0) { what_p = 0u; where = num++; sc = scale[p]; }
        else if (p < d) { what_p = 1u; where = cat++; }
        else if (num < dn4) { what_p = 2u; where = num++; }
        else { what_p = 3u; where = cat++; }
        s.w[2u * s.count] = (what_p << 30) | where;
        memcpy(&s.w[2u * s.count + 1u], &sc, 4);
        if (++s.count == D3P_PM_SLOTS || p + 1u == ns) {
            hipLaunchKernelGGL(k_mixed_schema, dim3(1), dim3(D3P_PM_SLOTS), 0, stream, s);
            if (const int rc = check_launch(what)) return rc;
            s.base += s.count;
            s.count = 0u;
        }
    }
    return D3P_OK;
}

static int mx_pack(const char* what, hipStream_t stream, const void* x, int32_t dtype, int64_t ld, uint32_t n, uint32_t d, uint32_t dn, uint32_t dc,
                   const uint32_t* slot, uint32_t* packed, uint32_t* flag)
{
    MxPackArgs p;
    p.x = static_cast<const uint32_t*>(x); p.ld = ld; p.n = n; p.d = d; p.ns = (uint32_t)mx_positions(dn, dc);
    p.pw = (uint32_t)mx_packed_words(dn, dc); p.dn4 = mx_num_words(dn); p.dtype = dtype;
    p.lw = 2;
    while (p.lw < 6 && (1u << p.lw) < p.ns) ++p.lw;
    p.slot = slot; p.packed = packed; p.flag = flag;
    const uint32_t rows = 256u >> p.lw;
    hipLaunchKernelGGL(k_mixed_pack, dim3((unsigned)(((uint64_t)n + rows - 1u) / rows)), dim3(256), 0, stream, p);   // <= 2^30 groups
    return check_launch(what);
}

}  // namespace d3p

using namespace d3p;

extern "C" {

uint32_t d3p_pair_stats_mixed_segment_tiles(void) { return D3P_PM_G; }

uint64_t d3p_pair_mixed_packed_words(uint32_t dn, uint32_t dc) { return mx_packed_words(dn, dc); }

uint32_t d3p_pair_stats_mixed_form(uint32_t na, uint32_t nb, uint32_t d) { return mx_form(na, nb, d); }

size_t d3p_pair_stats_mixed_workspace(uint32_t na, uint32_t nb, uint32_t dn, uint32_t dc) { return mx_layout(na, nb, dn, dc).total; }

// float64 additions on a row's sum: a lane's 4 pairs x G / 4 tiles of a segment, the butterfly's 3, the 4 slots, the segments
uint32_t d3p_pair_stats_mixed_roundings(uint32_t nb) { return nb < 1 ? 0u : D3P_PM_G + 3u + D3P_PAIR_WAVES + mx_segments(nb); }

int d3p_pair_stats_mixed_set_form(int32_t form) { return pair_set_form("d3p_pair_stats_mixed_set_form", form, &g_pm_form); }

int d3p_pair_stats_mixed(void* stream, const void* a_dev, const void* b_dev, int32_t dtype, int64_t a_ld, int64_t b_ld, uint32_t na, uint32_t nb,
                         uint32_t d, const uint8_t* kind, const float* scale, float w_cat, int32_t exclude_diagonal, double* sum_dev,
                         float* min_dev, uint32_t* argmin_dev, void* ws_dev, size_t ws_bytes)
{
    const char* what = "d3p_pair_stats_mixed";
    if (!a_dev || !b_dev || !kind || !scale || !sum_dev || !min_dev || !argmin_dev) return fail(D3P_E_INVALID_ARG, "%s: null pointer", what);
    if ((((uintptr_t)a_dev | (uintptr_t)b_dev | (uintptr_t)scale | (uintptr_t)min_dev | (uintptr_t)argmin_dev) & 3u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: a pointer is not aligned to 4 bytes", what);
    if ((((uintptr_t)sum_dev | (uintptr_t)ws_dev) & 7u) != 0)
        return fail(D3P_E_INVALID_ARG, "%s: sum_dev or ws_dev is not aligned to 8 bytes", what);
    if (const int rc = pair_check_pair(what, dtype, a_ld, b_ld, na, nb, d)) return rc;
    uint32_t dn = 0;
    for (uint32_t c = 0; c < d; ++c) {
        if (kind[c] > 1) return fail(D3P_E_INVALID_ARG, "%s: kind[%u] must be 0 (numeric) or 1 (categorical), got %u", what, c, (unsigned)kind[c]);
        dn += kind[c] == 0;
    }
    for (uint32_t c = 0; c < d; ++c)
        if (kind[c] == 0 && !(scale[c] >= 0.0f && std::isfinite(scale[c])))
            return fail(D3P_E_INVALID_ARG, "%s: scale[%u] must be finite and >= 0", what, c);
    if (!(w_cat >= 0.0f && std::isfinite(w_cat))) return fail(D3P_E_INVALID_ARG, "%s: w_cat must be finite and >= 0", what);
    if (const int rc = pair_check_diagonal(what, exclude_diagonal, na, nb)) return rc;
    const uint32_t dc = d - dn;
    const uint32_t form = mx_form(na, nb, d);
    const MxLayout l = mx_layout(na, nb, dn, dc);
    if (d <= D3P_PM_MAX_D && (ws_bytes < l.total || !ws_dev))
        return fail(D3P_E_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, ws_dev ? ws_bytes : (size_t)0, l.total);
    const uint64_t groups = (uint64_t)pair_tiles(na) * (form == D3P_PAIR_FORM_SPLIT ? mx_segments(nb) : 1u);
    if (groups > 0x7fffffffull) return fail(D3P_E_UNSUPPORTED, "%s: more than 2^31 - 1 workgroups (one per tile of a and segment of b)", what);
    if (d > D3P_PM_MAX_D) return fail(D3P_E_UNSUPPORTED, "%s: d above 2^28 (a packed position is 30 bits of a word)", what);
    if (!is_device_ptr(a_dev) || !is_device_ptr(b_dev) || !is_device_ptr(sum_dev) || !is_device_ptr(min_dev) || !is_device_ptr(argmin_dev) ||
        !is_device_ptr(ws_dev))
        return fail(D3P_E_INVALID_ARG, "%s: the tables, the outputs and the workspace must be device memory", what);
    char* ws = static_cast<char*>(ws_dev);
    uint32_t* slot = reinterpret_cast<uint32_t*>(ws + l.slot);
    uint32_t* pa = reinterpret_cast<uint32_t*>(ws + l.pa);
    uint32_t* pb = reinterpret_cast<uint32_t*>(ws + l.pb);
    uint32_t* fa = reinterpret_cast<uint32_t*>(ws + l.fa);
    uint32_t* fb = reinterpret_cast<uint32_t*>(ws + l.fb);
    if (const int rc = mx_upload_schema(what, (hipStream_t)stream, kind, scale, d, dn, dc, slot)) return rc;
    if (const int rc = mx_pack(what, (hipStream_t)stream, a_dev, dtype, a_ld, na, d, dn, dc, slot, pa, fa)) return rc;
    if (const int rc = mx_pack(what, (hipStream_t)stream, b_dev, dtype, b_ld, nb, d, dn, dc, slot, pb, fb)) return rc;
    MxArgs a;
    a.a = pa; a.b = pb; a.aflag = fa; a.bflag = fb; a.na = na; a.nb = nb; a.pw = (uint32_t)mx_packed_words(dn, dc); a.dn4 = mx_num_words(dn);
    a.excl = (uint32_t)exclude_diagonal; a.nseg = mx_segments(nb); a.w_cat = w_cat;
    a.sum = sum_dev; a.min = min_dev; a.argmin = argmin_dev;
    const size_t cells = (size_t)a.nseg * na;
    a.ws_sum = reinterpret_cast<double*>(ws);
    a.ws_min = l.cells ? reinterpret_cast<unsigned long long*>(ws + 8u * cells) : nullptr;
    a.ws_flag = l.cells ? reinterpret_cast<uint32_t*>(ws + 16u * cells) : nullptr;
    if (form == D3P_PAIR_FORM_WIDE) {
        hipLaunchKernelGGL(k_pair_mixed<D3P_PAIR_FORM_WIDE>, dim3((unsigned)groups), dim3(64 * D3P_PAIR_WAVES), 0, (hipStream_t)stream, a);
        return check_launch(what);
    }
    return pair_launch_merged(what, k_pair_mixed<D3P_PAIR_FORM_SPLIT>, k_pair_mixed_merge, (unsigned)groups, na, (hipStream_t)stream, a);
}

}  // extern "C"
