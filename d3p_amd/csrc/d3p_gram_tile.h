// The Gram walk on the matrix cores and what its two walkers share, one definition each: the Gaussian-kernel row sums (d3p_mmd.hip,
// DESIGN.md 4ze) and the soft-min rows (d3p_sinkhorn.hip, 4zf).  Both form, for a strip of rows of a table a and every row of a table b,
//     t_c  = fl32(fl32(x_c - shift_c) * scale_c)                        (one IEEE subtraction, one IEEE multiplication, never fused)
//     g_ij = sum_c ta_ic tb_jc                                          (v_mfma_f32_32x32x2_f32, float32 accumulator)
// and hand the 32 x 32 accumulator of a tile to an EPILOGUE, the part that varies.  Here: the constants of the geometry, the value, the
// flag and the t of a loaded word, the load / store pair that stages a tile, the walk over the tiles of a segment (gram_walk: the
// double-buffered staging, the resident or streaming operands of a, the product loop, the norm of b a tile ahead, the flags) and --
// HOST, at the end -- the segment rule and the host steps of the two entries (gram_prepare, gram_launch_norms).  d3p_mmd.hip's header states the order of g and the layout in full; this file is that text's
// code.  What a walker's argument struct must carry under these names (ARGS): a, b (uint32_t words), dtype, a_ld, b_ld, na, nb, d, nseg,
// tps, vec_a, vec_b, shift, scale, ra, rb.  An EPILOGUE (EPI) has
//     ahead(j, live)     the loads of column j that ride with rb_j, issued a tile ahead (live: j < nb and inside the segment)
//     advance()          the tile ahead becomes the current one
//     tile(acc, ra, rb, r0, half, j, k, last, red, lane)   the 16 x 32 pairs of lane (half, sub = j % 32) of the segment's k-th tile
//     bad()              a flag of its own loads, for every row (as one in b)
#pragma once
#include "d3p_device.h"
#include "d3p_pair_tile.h"

#define D3P_GRAM_WAVES 4u
#define D3P_GRAM_TILE 32u                                 // rows of a wavefront, rows of a tile of b
#define D3P_GRAM_STRIP (D3P_GRAM_WAVES * D3P_GRAM_TILE)   // rows of a workgroup
#define D3P_GRAM_CHUNK 32u                                // columns staged at a time by the streaming form
#define D3P_GRAM_RES 64u                                  // d up to which the A operands stay in registers
#define D3P_GRAM_TARGET 1024u                             // workgroups the segment rule aims at
#define D3P_GRAM_RED 33u                                  // row pitch of the group-end transpose

namespace d3p {

typedef float gram_f16v __attribute__((ext_vector_type(16)));

struct GramTable { const uint32_t* base; int64_t ld; uint32_t n, vec; };

// STATIC LDS of a walk: RES 16640 + 16896 + 516 = 34052 bytes (+ 8 of a one-word stand-in for `as`); streaming 8448 + 33792 + 16896 + 516
template <bool RES>
struct GramLds {
    static constexpr uint32_t KW = RES ? D3P_GRAM_RES : D3P_GRAM_CHUNK, PITCH = KW + 1u;
    float bs[2][D3P_GRAM_TILE * PITCH];
    float as[2][RES ? 1u : D3P_GRAM_STRIP * PITCH];
    float red[D3P_GRAM_WAVES][D3P_GRAM_TILE * D3P_GRAM_RED];
    uint32_t aflag[D3P_GRAM_STRIP];
    uint32_t bflag;
};

__device__ __forceinline__ float gram_value(int32_t dtype, uint32_t w) { return dtype ? (float)(int32_t)w : __uint_as_float(w); }
__device__ __forceinline__ bool gram_not_finite(float v) { return !(fabsf(v) <= 3.402823466e38f); }

// THE t of one element in column c < d
__device__ __forceinline__ float gram_t(float v, float sh, float sc, bool shifted, bool scaled)
{
#pragma clang fp contract(off)
    float t = v;
    if (shifted) t = t - sh;
    if (scaled) t = t * sc;
    return t;
}

// THE norm of row `x`: the float32 chain r <- fmaf(t_c, t_c, r) over c ascending from +0 (a thread per row)
template <class ARGS>
__device__ __forceinline__ float gram_norm(const ARGS& a, const uint32_t* x)
{
    float r = 0.0f;
    for (uint32_t c = 0; c < a.d; ++c) {
        const float t = gram_t(gram_value(a.dtype, x[c]), a.shift ? a.shift[c] : 0.0f, a.scale ? a.scale[c] : 1.0f, a.shift != nullptr, a.scale != nullptr);
        r = __fmaf_rn(t, t, r);
    }
    return r;
}

// the norms launch's body: thread idx < na + nb writes r of its row to a.ra or a.rb
template <class ARGS>
__device__ __forceinline__ void gram_norms(const ARGS& a)
{
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)a.na + a.nb) return;
    const bool second = idx >= a.na;
    const uint64_t row = second ? idx - a.na : idx;
    (second ? a.rb : a.ra)[row] = gram_norm(a, (second ? a.b : a.a) + (int64_t)row * (second ? a.b_ld : a.a_ld));
}

// 2^lw >= units threads share a row, lw >= 3 (a tile of 32 rows is then one pass of the 256 threads at the least)
__device__ __forceinline__ uint32_t gram_lanes_log2(uint32_t units) { return units > 32u ? 6u : units > 16u ? 5u : units > 8u ? 4u : 3u; }

// Thread t of 256 takes UNIT u = t % 2^lw -- four columns from c0 + 4 u with the 16-byte loads, else column c0 + u -- of the rows
// row0 + t / 2^lw + p (256 / 2^lw) of `rows` rows: up to NW words.  A dead row reads the table's last row, a dead column column 0: every
// load is inside the table and none sits behind a divergent branch.
template <uint32_t NW>
__device__ __forceinline__ void gram_load(const GramTable& T, uint32_t row0, uint32_t rows, uint32_t c0, uint32_t d, uint32_t lw, uint32_t t,
                                          uint32_t (&w)[NW])
{
    const uint32_t u = t & ((1u << lw) - 1u), rl = t >> lw, rpp = 256u >> lw, passes = rows / rpp;
    if (T.vec) {
        const uint32_t c = c0 + 4u * u, cr = c < d ? c : 0u;   // (c < d: c + 3 < ld, both multiples of 4)
#pragma unroll
        for (uint32_t p = 0; p < NW / 4u; ++p) {
            if (p < passes) {
                const uint32_t row = row0 + rl + p * rpp;
                const uint4 v = *reinterpret_cast<const uint4*>(T.base + (int64_t)(row < T.n ? row : T.n - 1u) * T.ld + cr);
                w[4u * p] = v.x; w[4u * p + 1u] = v.y; w[4u * p + 2u] = v.z; w[4u * p + 3u] = v.w;
            }
        }
    } else {
        const uint32_t c = c0 + u, cr = c < d ? c : 0u;
#pragma unroll
        for (uint32_t p = 0; p < NW; ++p) {
            if (p < passes) {
                const uint32_t row = row0 + rl + p * rpp;
                w[p] = T.base[(int64_t)(row < T.n ? row : T.n - 1u) * T.ld + cr];
            }
        }
    }
}

// shift and scale of the unit's columns (0 and 1 where the pointer is null or the column dead: gram_t does not read them then)
template <class ARGS>
__device__ __forceinline__ void gram_coeffs(const ARGS& a, uint32_t vec, uint32_t c0, uint32_t u, float (&sh)[4], float (&sc)[4])
{
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) {
        const uint32_t c = vec ? c0 + 4u * u + e : c0 + u, cr = c < a.d ? c : 0u;
        sh[e] = a.shift ? a.shift[cr] : 0.0f;
        sc[e] = a.scale ? a.scale[cr] : 1.0f;
    }
}

// the words of gram_load as t into lds[row * pitch + column - c0]: units below `units` only; a dead row or column is 0 (by select, after
// the arithmetic); a live element that is NaN or +-inf sets `bad` and, with rowflag, its row's word
template <uint32_t NW, class ARGS>
__device__ __forceinline__ void gram_store(const ARGS& a, const GramTable& T, uint32_t row0, uint32_t rows, uint32_t c0, uint32_t lw, uint32_t units,
                                           uint32_t t, const uint32_t (&w)[NW], const float (&sh)[4], const float (&sc)[4], float* lds, uint32_t pitch,
                                           uint32_t* rowflag, bool& bad)
{
    const uint32_t u = t & ((1u << lw) - 1u), rl = t >> lw, rpp = 256u >> lw, passes = rows / rpp;
    const uint32_t per = T.vec ? 4u : 1u;
    if (u >= units) return;
#pragma unroll
    for (uint32_t p = 0; p < NW; ++p) {
        const uint32_t pass = T.vec ? p >> 2 : p, e = T.vec ? p & 3u : 0u;
        if (pass < passes) {
            const uint32_t lr = rl + pass * rpp, lc = per * u + e;
            const bool live = row0 + lr < T.n && c0 + lc < a.d;
            const float v = gram_value(a.dtype, w[p]);
            const bool nf = live && gram_not_finite(v);
            bad |= nf;
            if (rowflag && nf) rowflag[lr] = 1u;
            const float tv = gram_t(v, sh[e], sc[e], a.shift != nullptr, a.scale != nullptr);
            lds[lr * pitch + lc] = live ? tv : 0.0f;
        }
    }
}

// the row of the accumulator's register v in lane (half, .): lane (half, sub) holds the rows 8 (v / 4) + 4 half + v % 4 of column sub
__device__ __forceinline__ uint32_t gram_acc_row(uint32_t v, uint32_t half) { return 8u * (v >> 2) + 4u * half + (v & 3u); }

// THE WALK of one workgroup (256 threads: a strip of 128 rows of a, 32 per wavefront, and segment `seg` of b) with epilogue `epi`.
// Returns, in the lanes below 32, the flag word of row r0 + lane (pair_flag_word: the row's own flag, the flag of b and of the epilogue's
// loads); ends behind a barrier.
template <bool RES, class ARGS, class EPI>
__device__ __forceinline__ uint32_t gram_walk(const ARGS& a, GramLds<RES>& L, EPI& epi)
{
    constexpr uint32_t PITCH = GramLds<RES>::PITCH, NWB = RES ? 8u : 4u, NWA = RES ? 1u : 16u;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, half = lane >> 5, sub = lane & 31u;
    const uint32_t strip = pair_split_tile(a.nseg), seg = pair_split_segment(a.nseg);
    const uint32_t s0 = strip * D3P_GRAM_STRIP, r0 = s0 + wave * D3P_GRAM_TILE;     // (na < 2^31: no wrap)
    const uint32_t ntb = pair_tiles(a.nb), j_lo = seg * a.tps, j_hi = ntb - j_lo < a.tps ? ntb : j_lo + a.tps;
    const uint32_t nchunk = RES ? 1u : (a.d + D3P_GRAM_CHUNK - 1u) / D3P_GRAM_CHUNK, nq = (a.d + 1u) / 2u;
    const GramTable ta = {a.a, a.a_ld, a.na, a.vec_a}, tb = {a.b, a.b_ld, a.nb, a.vec_b};
    // the units of a staged row: RES all d columns of b (to an even count: the pair 2 p, 2 p + 1), else a chunk of 32
    const uint32_t ub = RES ? (tb.vec ? (a.d + 3u) / 4u : 2u * nq) : (tb.vec ? 8u : 32u), lwb = gram_lanes_log2(ub);
    const uint32_t ua = ta.vec ? 8u : 32u, lwa = ta.vec ? 3u : 5u;
    if (t < D3P_GRAM_STRIP) L.aflag[t] = 0u;
    if (t == 0u) L.bflag = 0u;
    __syncthreads();

    bool bad_a = false, bad_b = false;
    float areg[RES ? D3P_GRAM_RES / 2u : 1u];
    if constexpr (RES) {   // lane (half, sub) holds column 2 p + half of row r0 + sub
        const uint32_t row = r0 + sub;
        const uint32_t* x = a.a + (int64_t)(row < a.na ? row : a.na - 1u) * a.a_ld;
#pragma unroll
        for (uint32_t p = 0; p < D3P_GRAM_RES / 2u; ++p) {
            areg[p] = 0.0f;
            if (p < nq) {   // (uniform)
                const uint32_t c = 2u * p + half, cr = c < a.d ? c : 0u;
                const bool live = row < a.na && c < a.d;
                const float v = gram_value(a.dtype, x[cr]);
                bad_a |= live && gram_not_finite(v);
                const float tv = gram_t(v, a.shift ? a.shift[cr] : 0.0f, a.scale ? a.scale[cr] : 1.0f, a.shift != nullptr, a.scale != nullptr);
                areg[p] = live ? tv : 0.0f;
            }
        }
    }
    float ra[16];
#pragma unroll
    for (uint32_t v = 0; v < 16u; ++v) {
        const uint32_t i = r0 + gram_acc_row(v, half);
        ra[v] = a.ra[i < a.na ? i : a.na - 1u];
    }

    uint32_t wb[NWB], wa[NWA];
    float shb[4], scb[4], sha[4], sca[4];
    auto load = [&](uint32_t J, uint32_t c0) {
        gram_load<NWB>(tb, J * D3P_GRAM_TILE, D3P_GRAM_TILE, c0, a.d, lwb, t, wb);
        if constexpr (!RES) {
            gram_load<NWA>(ta, s0, D3P_GRAM_STRIP, c0, a.d, lwa, t, wa);
            gram_coeffs(a, tb.vec, c0, t & ((1u << lwb) - 1u), shb, scb);
            gram_coeffs(a, ta.vec, c0, t & ((1u << lwa) - 1u), sha, sca);
        }
    };
    auto store = [&](uint32_t J, uint32_t c0, uint32_t buf) {
        gram_store<NWB>(a, tb, J * D3P_GRAM_TILE, D3P_GRAM_TILE, c0, lwb, ub, t, wb, shb, scb, L.bs[buf], PITCH, nullptr, bad_b);
        if constexpr (!RES) gram_store<NWA>(a, ta, s0, D3P_GRAM_STRIP, c0, lwa, ua, t, wa, sha, sca, L.as[buf], PITCH, L.aflag, bad_a);
    };

    if constexpr (RES) gram_coeffs(a, tb.vec, 0u, t & ((1u << lwb) - 1u), shb, scb);
    const bool live0 = j_lo * D3P_GRAM_TILE + sub < a.nb;
    float rb_next = live0 ? a.rb[j_lo * D3P_GRAM_TILE + sub] : 0.0f;
    epi.ahead(j_lo * D3P_GRAM_TILE + sub, live0);
    load(j_lo, 0u);
    uint32_t step = 0u;
    for (uint32_t J = j_lo; J < j_hi; ++J) {
        const float rb = rb_next;
        epi.advance();
        {
            const uint32_t jn = (J + 1u) * D3P_GRAM_TILE + sub;
            const bool live = J + 1u < j_hi && jn < a.nb;
            rb_next = live ? a.rb[jn] : 0.0f;
            epi.ahead(jn, live);
        }
        gram_f16v acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
        for (uint32_t c = 0; c < nchunk; ++c, ++step) {
            const uint32_t buf = step & 1u;
            store(J, c * D3P_GRAM_CHUNK, buf);
            __syncthreads();   // ONE a step: this buffer was last read two steps ago, before the barrier of the step between
            if (c + 1u < nchunk) load(J, (c + 1u) * D3P_GRAM_CHUNK);
            else if (J + 1u < j_hi) load(J + 1u, 0u);
            const float* brow = L.bs[buf] + sub * PITCH + half;
            if constexpr (RES) {
#pragma unroll
                for (uint32_t p = 0; p < D3P_GRAM_RES / 2u; ++p)
                    if (p < nq) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[p], brow[2u * p], acc, 0, 0, 0);   // (uniform)
            } else {
                const float* arow = L.as[buf] + (wave * D3P_GRAM_TILE + sub) * PITCH + half;
#pragma unroll
                for (uint32_t p = 0; p < D3P_GRAM_CHUNK / 2u; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2u * p], brow[2u * p], acc, 0, 0, 0);
            }
        }
        epi.tile(acc, ra, rb, r0, half, J * D3P_GRAM_TILE + sub, J - j_lo, J + 1u == j_hi, L.red[wave], lane);
    }

    const unsigned long long abits = __builtin_amdgcn_ballot_w64(bad_a);   // RES: lanes r and r + 32 loaded row r
    if (bad_b || epi.bad()) L.bflag = 1u;
    __syncthreads();
    const uint32_t fa = RES ? (uint32_t)(((abits >> (lane & 31u)) | (abits >> ((lane & 31u) + 32u))) & 1ull) : L.aflag[wave * D3P_GRAM_TILE + (lane & 31u)];
    return pair_flag_word(fa, L.bflag);
}

// ------------------------------------------------------------------------------------------------ HOST

static const uint32_t GRAM_MAX_N = 0x7fffffffu;

inline uint32_t gram_strips(uint32_t na) { return (uint32_t)(((uint64_t)na + D3P_GRAM_STRIP - 1u) / D3P_GRAM_STRIP); }

inline bool gram_sizes_ok(uint32_t na, uint32_t nb) { return na >= 1 && nb >= 1 && na <= GRAM_MAX_N && nb <= GRAM_MAX_N; }

// THE segment rule: tiles of b per segment from (na, nb) alone (and the walker's forced count, 0 = the rule): nseg = min(tiles of b,
// ceil(1024 / strips)) segments of ceil(tiles / nseg) tiles
inline uint32_t gram_segment_tiles(uint32_t na, uint32_t nb, int32_t forced)
{
    const uint32_t ntb = pair_tiles(nb), strips = gram_strips(na);
    uint32_t want = forced > 0 ? (uint32_t)forced : (D3P_GRAM_TARGET + strips - 1u) / strips;
    if (want > ntb) want = ntb;
    return (ntb + want - 1u) / want;
}

inline uint32_t gram_segments(uint32_t na, uint32_t nb, int32_t forced)
{
    if (!gram_sizes_ok(na, nb)) return 0;
    const uint32_t tps = gram_segment_tiles(na, nb, forced);
    return (pair_tiles(nb) + tps - 1u) / tps;
}

// What an entry does between the refusals of its own arguments and that of its workspace (the tables have passed pair_check_pair):
// the refusals of the sizes, the geometry under the entry's forced segment count, and the fields of ARGS that gram_walk and
// gram_norms read but ra and rb, which the entry carves from its workspace.  Returns the workgroups of the walk, one per strip of a
// and segment of b -- or 0 behind a refusal, which is D3P_E_UNSUPPORTED with the message set
template <class ARGS>
inline unsigned gram_prepare(const char* what, int32_t forced, const void* a_dev, const void* b_dev, int32_t dtype, int64_t a_ld, int64_t b_ld,
                             uint32_t na, uint32_t nb, uint32_t d, const float* shift_dev, const float* scale_dev, ARGS& a)
{
    if (na > GRAM_MAX_N || nb > GRAM_MAX_N) {
        fail(D3P_E_UNSUPPORTED, "%s: %u x %u rows; at most 2^31 - 1 each", what, na, nb);
        return 0;
    }
    const uint32_t tps = gram_segment_tiles(na, nb, forced), nseg = gram_segments(na, nb, forced);
    const uint64_t groups = (uint64_t)gram_strips(na) * nseg;
    if (groups > 0x7fffffffull) {
        fail(D3P_E_UNSUPPORTED, "%s: more than 2^31 - 1 workgroups (one per strip of a and segment of b)", what);
        return 0;
    }
    a.a = static_cast<const uint32_t*>(a_dev); a.b = static_cast<const uint32_t*>(b_dev); a.dtype = dtype; a.a_ld = a_ld; a.b_ld = b_ld;
    a.na = na; a.nb = nb; a.d = d; a.nseg = nseg; a.tps = tps;
    a.vec_a = ((uintptr_t)a_dev & 15u) == 0 && (a_ld & 3) == 0; a.vec_b = ((uintptr_t)b_dev & 15u) == 0 && (b_ld & 3) == 0;
    a.shift = shift_dev; a.scale = scale_dev;
    return (unsigned)groups;
}

// the first launch of both entries: a walker's norms kernel (gram_norms), a thread per row of a and of b
template <class ARGS>
inline int gram_launch_norms(const char* what, void (*norms)(ARGS), hipStream_t stream, const ARGS& a)
{
    hipLaunchKernelGGL(norms, dim3((unsigned)(((uint64_t)a.na + a.nb + 255u) / 256u)), dim3(256), 0, stream, a);
    return check_launch(what);
}

}  // namespace d3p
