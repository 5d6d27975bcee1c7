// The strided matrix-product layer of the VAE step (d3p_gemm.hip): what d3p_vae.hip needs of it.
#pragma once
#include "d3p_device.h"
#include "d3p_host.h"

namespace d3p {

struct GemmJumps {  // see GemmArgs::n_seg
    int n_seg, k_seg;
    long long b_njump, b_kjump, bias_njump, c_njump;
};

struct GemmArgs {
    const float* A;
    const float* B;
    float* C;
    const float* bias;  // nullable, length N
    int M, N, K;
    long long a_sm, a_sk, b_sk, b_sn;
    int ldc;
    float alpha;
    int accumulate;
    int a_last_one;   // row M - 1 of op(A) is all ones (bias gradients ride along with the weight gradients)
    int k_per;        // K range of one split (multiple of D3P_GK); gridDim.z splits
    float* part;      // split-K partial tiles [gridDim.z][M][N] (nullable when gridDim.z == 1)
    int epi;          // epilogue: 0 store; 1 softplus (C = softplus(o), C2 = sigmoid(o) = its derivative); 2 C = o * C2;
                      // 3 (the dz product, C = [dz | du] of row stride 2 Z): dz = o + sc z, du = dz sd eps - sc with [z | sd] = ex_zu (same
                      // layout as C), eps dense B x Z (the backward pass through the reparametrised latent, svi.py:289-290 draw)
                      // 4 (k_gemm_bf16x3<.., EPI4> only; the decoder's output layer, C = logits B x D): what k_vae_out does in a launch of
                      // its own -- C = sc (sigmoid(o) - x) with x = ep_x (the batch, laid out like C; requested BEFORE the K loop: at
                      // the end the tile's 32 KB would arrive in one burst with nothing left to overlap), and per row and group of 32
                      // columns (one wave's share) the partial sums of x o - softplus(o) and of x^2 in ep_ll / ep_xx
                      // ([ceil(N / 32)][M]), summed in fixed order (DPP) -- the norm kernel adds the groups (vae_out_finish_row)
    const float* ex_zu;
    const float* ex_eps;
    int ex_Z;
    float ex_sc;
    const float* ep_x;
    float* ep_ll;
    float* ep_xx;
    // Two operands side by side that are not adjacent in memory (the pairs (Wl, Ws) / (bl, bs) of the flat parameter layout lie
    // H Z apart): columns n >= n_seg of B, of the bias and of C, and rows k >= k_seg of B, are displaced by a constant.  0 / 0 /
    // INT_MAX segments = plain GEMM.  Honoured by the scalar B fetch and by every store path.
    int n_seg, k_seg;
    long long b_njump, b_kjump, bias_njump, c_njump;
    float* C2;        // second operand / output of the epilogue, same shape and leading dimension as C
    // k_gemm_bf16x3 only, nullable: a device word that is non-zero when EVERY element of A is exactly a bf16 number (low 16 bits of
    // the fp32 pattern zero) -- binarised images (examples/vae.py:157-168), one-hot rows, small integers.  The second and third
    // plane of A are then exactly zero: the kernel stages plane 0 alone (no splitting of A) and issues the three products with a_0
    // (of six); the sums are those of the general path (the dropped products are exact zeros, the others come in the same order).
    const uint32_t* a_exact16;
    // k_gemm_bf16x3 with an n-fast B only, nullable: row k of B is multiplied by b_row_scale[k] while it is staged (the clip factors
    // of the weight-gradient products: B = a delta array, k = the example -- svi.py:121-122 folded into the sum; the fp32 product
    // c_k b is rounded once, as if the scaled rows had been written to memory and read back)
    const float* b_row_scale;
    uint32_t a_exact_nonce;   // A is exact iff *a_exact16 != a_exact_nonce: the checking pass stores the nonce of ITS pass when it finds an
                              // inexact element, so the word needs no reset between passes (whatever it held before, a stale match can
                              // only send an exact batch down the general path)
};

// the flag of GemmArgs::a_exact16 for an array of n floats (n a multiple of 4, 16-byte aligned): 1 unless some element has low bits
__device__ __forceinline__ void exact16_pass(const float* __restrict__ x, size_t n4, uint32_t* __restrict__ flag, uint32_t nonce, unsigned block,
                                             unsigned n_blocks)
{
    uint32_t bad = 0u;
    for (size_t i = (size_t)block * blockDim.x + threadIdx.x; i < n4; i += (size_t)n_blocks * blockDim.x) {
        const uint4 v = reinterpret_cast<const uint4*>(x)[i];
        bad |= (v.x | v.y | v.z | v.w) & 0xffffu;
    }
    if (__ballot(bad != 0u) != 0ull && (threadIdx.x & 63) == 0) *flag = nonce;   // (every writer writes the same value)
}

// the exactness pass as a launch of its own (k_exact16_flag), and its grid
inline unsigned exact16_blocks(size_t n4) { return (unsigned)(n4 / 1024 < 1 ? 1 : (n4 / 1024 > 1024 ? 1024 : n4 / 1024)); }
void exact16_flag_launch(hipStream_t s, const float* x, size_t n4, uint32_t* flag, uint32_t nonce);

#define D3P_GT 64    // tile edge (k_gemm_f32; N edge of the eight-wave kernels)
#define D3P_GK 16    // K slice of k_gemm_f32
#define D3P_GTM 128  // M edge and K slice of the eight-wave kernels (k_gemm_f32_w8, k_gemm_bf16x3)
#define D3P_GKB 32

// Several products of one operand form in ONE launch (the weight-gradient products of a step: independent of each other, each too
// short to fill the chip for a whole number of rounds -- 112 / 468 / 490 / 128 workgroups on 256 CUs -- and each paying its own
// launch floor): a linear grid over the workgroups of all members, dealt to the XCDs as xcd_tile deals one product's (every XCD
// walks one contiguous run of the order member, K slab, m, n), the host choosing ONE K range per workgroup for all members so that
// the run is a whole number of equal rounds (gemm_group_splits).
// (D3P_GROUP_MAX members at most: include/d3p_hip.h)
#define D3P_WPART_SPLITS 16  // most split-K partial tiles a product leaves
struct GemmGroup {
    GemmArgs g[D3P_GROUP_MAX];
    // Every XCD takes one contiguous eighth of EVERY member, member after member (so the XCDs work through the members in step --
    // one run over all members would give some XCDs only the cheap ones): slot[p] = first per-XCD slot of member p (its share is
    // slot[p + 1] - slot[p] = ceil(cnt[p] / 8) workgroups per XCD; the up to 7 surplus workgroups of a member leave at once)
    unsigned slot[D3P_GROUP_MAX + 1];
    unsigned cnt[D3P_GROUP_MAX];         // workgroups of member p = gx gy splits
    unsigned gx[D3P_GROUP_MAX], gy[D3P_GROUP_MAX];
    // one more workgroup behind the members', when asked for: *sum_out = sum of sum_in[0 .. sum_n - 1] in fixed order (the loss sum of
    // a step whose output layer was fused -- NormArgs: the norm kernel in front of this launch completes px_loss, so it cannot sum it)
    const float* sum_in;
    float* sum_out;
    unsigned sum_n;
};

// members collected by gemm() instead of being launched (its `group` argument), then launched together
struct GemmGroupPlan {
    GemmGroup q;
    int n = 0;
    bool ak = false, bn = false;
    const float* sum_in = nullptr;   // GemmGroup::sum_in / sum_out / sum_n
    float* sum_out = nullptr;
    unsigned sum_n = 0;
};

// what gemm() decides for a product (gemm_route; GemmOpts::report)
enum { GEMM_ROUTE_F32 = D3P_GEMM_ROUTE_F32, GEMM_ROUTE_F32_VA = D3P_GEMM_ROUTE_F32_VA, GEMM_ROUTE_F32_VB = D3P_GEMM_ROUTE_F32_VB, GEMM_ROUTE_W8 = D3P_GEMM_ROUTE_W8,
       GEMM_ROUTE_BF16X3 = D3P_GEMM_ROUTE_BF16X3, GEMM_ROUTE_GROUPED = D3P_GEMM_ROUTE_GROUPED };
struct GemmReport {
    int route;    // k_gemm_f32<VA, VB>: GEMM_ROUTE_F32 | VA bit | VB bit; otherwise one of the other values
    int splits;   // K slabs of the launch (gridDim.z)
};

// what a product may ask for beyond C = alpha op(A) op(B) + bias (+ C); every field optional
struct GemmOpts {
    int a_last_one = 0;             // GemmArgs::a_last_one
    float* part = nullptr;          // split-K scratch ([splits][M][N]) and its size: without it the product is not split
    size_t part_floats = 0;
    int epi = 0;                    // GemmArgs::epi and its operands
    float* C2 = nullptr;
    const float* ex_zu = nullptr;
    const float* ex_eps = nullptr;
    int ex_Z = 0;
    float ex_sc = 0.f;
    int* splits_left = nullptr;     // a split-K product is NOT reduced: the partial tiles stay in `part` and *splits_left says how many
                                    // (0: the product went to C as usual); the consumer sums them in fixed order
    const GemmJumps* jumps = nullptr;
    const uint32_t* a_exact16 = nullptr;   // GemmArgs::a_exact16 / a_exact_nonce
    uint32_t a_exact_nonce = 0u;
    GemmGroupPlan* group = nullptr; // (with splits_left) a product that takes the bf16 kernel is appended to the group instead of
    int force_splits = 0;           // being launched (gemm_group_launch), with force_splits K slabs instead of a count of its own
    const float* b_row_scale = nullptr;    // GemmArgs::b_row_scale: bf16 kernel with an n-fast B only (gemm_route)
    const float* ep_x = nullptr;    // epi 4 (with ex_sc): k-fast A, n-fast B on the bf16 kernel, unsplit (gemm_route)
    float *ep_ll = nullptr, *ep_xx = nullptr;
    GemmReport* report = nullptr;   // test aid (d3p_gemm_f32_ex): which kernel the product takes and its final split count
    bool plan_only = false;         // test aid: decide (refusals, report) and return before anything is appended or launched
};

// The kernel gemm() gives a product: GEMM_ROUTE_F32 | VA bit | VB bit, GEMM_ROUTE_W8 or GEMM_ROUTE_BF16X3 -- THE routing rule, also
// asked by whoever wants b_row_scale or epilogue 4 (they need GEMM_ROUTE_BF16X3 with b_sn == 1 and no displaced B segments).
int gemm_route(const float* A, long long a_sm, long long a_sk, const float* B, long long b_sk, long long b_sn, int M, int N, int K, int a_last_one,
               const GemmJumps* jumps);
int gemm_group_splits(unsigned tiles, int K);
int gemm(hipStream_t s, const float* A, long long a_sm, long long a_sk, const float* B, long long b_sk, long long b_sn, float* C, int ldc, int M, int N,
         int K, const float* bias, float alpha, int accumulate, const GemmOpts& o = GemmOpts());
int gemm_group_launch(hipStream_t s, GemmGroupPlan& G);

}  // namespace d3p
