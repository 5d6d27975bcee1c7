/*
 * d3p_hip.h -- C-ABI of libd3p_hip.so: the MI355X (gfx950) hot path of d3p's DP-VI update step.
 *
 * The reference (DPBayes/d3p 0.2.0) is pure Python; it has no FFI boundary of its own
 * (SURVEY.md F5).  Each entry point below replaces one Python-level call on the hot path and
 * cites it (file:line relative to the reference root).  INTEGRATION.md shows the ctypes stub a
 * d3p maintainer would add to route the reference's modules through this library.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no torch / HIP types in signatures
 *     (`stream` is a hipStream_t passed as void*, NULL = the default stream).
 *   - Every `*_dev` / device pointer is a raw device address (e.g. torch.Tensor.data_ptr()).
 *     The caller owns all memory; the library allocates nothing and keeps no references.
 *   - All calls are asynchronous on `stream`; nothing synchronises the device.
 *   - Return value: 0 = D3P_OK, negative = error; d3p_last_error() returns a thread-local
 *     message for the last failing call on this thread.
 *   - ChaCha20 keys ("PRNGState", d3p/random/__init__.py:28) are 16 x uint32 RFC 8439 states:
 *     [0..3] constants, [4..11] key, [12] counter, [13..15] nonce (layout: DESIGN.md section 3).
 *   - Threefry keys (d3p/random/debug.py, and the per-example guide noise) are 2 x uint32.
 */
#ifndef D3P_HIP_H
#define D3P_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D3P_OK 0
#define D3P_E_INVALID_ARG (-1)
#define D3P_E_HIP (-2)
#define D3P_E_UNSUPPORTED (-3)
#define D3P_E_WORKSPACE (-4)

#define D3P_ABI_VERSION 9
#define D3P_IPC_HANDLE_BYTES 80   /* what d3p_xchg_create / d3p_fmesh_create hand out for the peers (ABI 9) */

int d3p_abi_version(void);
const char* d3p_last_error(void);
/* Number of visible HIP devices (<= 0: none; the Python layer refuses to run without one). */
int d3p_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * rng_suite: ChaCha20 CSPRNG -- replaces chacha.random as aliased by d3p/random/__init__.py:28-32
 * and the functions d3p adds on top (:50-155).
 * ------------------------------------------------------------------------------------------- */
/* split(key, num) -> num keys   (d3p/random/__init__.py:29; svi.py:210, :491) */
int d3p_rng_split(void* stream, const uint32_t* key_dev, int num, uint32_t* out_keys_dev);
/* Host only (no device, no stream): the first num_links links of the key chain of DPSVI.update from `key` -- link t is
 * split(k_t, 3), k_0 = key, k_{t+1} = split(k_t, 3)[0].  out_keys: num_links x 3 x 16 words (children 0, 1, 2 of each link).
 * The derivation the runs' start uses for the links it prepares on the host; exported so that it can be checked without a GPU. */
int d3p_key_chain_host(const uint32_t* key, int num_links, uint32_t* out_keys);
/* fold_in(key, data)            (d3p/random/__init__.py:30; minibatch.py:115, :207, :230) */
int d3p_rng_fold_in(void* stream, const uint32_t* key_dev, uint32_t data, uint32_t* out_key_dev);
/* random_bits(key, bit_width in {8,16,32,64}, shape) -> `count` elements
 * (d3p/random/__init__.py:31; util.py:240-242).  out_dev must hold
 * ceil(count*bit_width/512) * 64 bytes (whole ChaCha blocks are written). */
int d3p_rng_random_bits(void* stream, const uint32_t* key_dev, int bit_width, uint64_t count,
                        void* out_dev);
/* uniform(key, shape, float32, minval, maxval)  (d3p/random/__init__.py:32, :80; minibatch.py:34) */
int d3p_rng_uniform(void* stream, const uint32_t* key_dev, uint64_t n, float minval, float maxval,
                    float* out_dev);
/* normal(key, shape, float32) = sqrt(2) * erf_inv(uniform(nextafter(-1,0), 1))
 * (d3p/random/__init__.py:50-81; svi.py:487) */
int d3p_rng_normal(void* stream, const uint32_t* key_dev, uint64_t n, float* out_dev);
/* randint(key, shape, minval, maxval, int32): masked rejection sampling
 * (d3p/random/__init__.py:84-146; minibatch.py:208) */
int d3p_rng_randint(void* stream, const uint32_t* key_dev, uint64_t n, int32_t minval,
                    int32_t maxval, int32_t* out_dev);

/* ---------------------------------------------------------------------------------------------
 * debug rng_suite: threefry2x32 in jax.random's array layout -- replaces d3p/random/debug.py:34-80.
 * The same generator produces the per-example guide noise (svi.py:259, :289-290).
 * ------------------------------------------------------------------------------------------- */
/* ABI 3: randint for the 8-, 16-, 32- and 64-bit integer dtypes (d3p/random/__init__.py:108-146, the dtype table at
 * :115-123; tests/test_random.py:74-135 draw int8 over the full range and int16 up to 2^15): delta and the power-of-two
 * mask are formed in the unsigned dtype of that width (float32 log2, :124-128), element j of random_bits(round_key, bit_width,
 * shape) is the little-endian bit_width-wide view of the keystream, the result wraps in the signed dtype.  out_dev holds n
 * elements of bit_width bits. */
int d3p_rng_randint_bits(void* stream, const uint32_t* key_dev, uint64_t n, int bit_width, int64_t minval, int64_t maxval,
                         void* out_dev);
int d3p_tf_split(void* stream, const uint32_t* key_dev, int num, uint32_t* out_keys_dev);
int d3p_tf_fold_in(void* stream, const uint32_t* key_dev, uint32_t data, uint32_t* out_key_dev);
int d3p_tf_random_bits(void* stream, const uint32_t* key_dev, uint64_t n_words, uint32_t* out_dev);
int d3p_tf_uniform(void* stream, const uint32_t* key_dev, uint64_t n, float minval, float maxval,
                   float* out_dev);
int d3p_tf_normal(void* stream, const uint32_t* key_dev, uint64_t n, float* out_dev);
/* jax.random.randint(key, shape, minval, maxval, int32) (d3p/random/debug.py:39) */
int d3p_tf_randint(void* stream, const uint32_t* key_dev, uint64_t n, int32_t minval, int32_t maxval,
                   int32_t* out_dev);

/* ---------------------------------------------------------------------------------------------
 * Workspaces (every entry below that takes `workspace_dev, workspace_bytes`; its size is the `d3p_*_workspace()` function
 * declared beside it, called with the same arguments).  The contents on entry are unspecified: whatever an entry reads --
 * accumulators, counters, flags, tagged words, status words -- it has initialised in the same call.  An entry writes nothing
 * outside [workspace_dev, workspace_dev + d3p_*_workspace()), however much larger workspace_bytes is.  A buffer shorter than
 * that size is refused with D3P_E_WORKSPACE before anything is launched: outputs, state and the buffer stay as they were.
 * What one run leaves in a workspace never changes what the next computes: the same arguments give the same output bits on a
 * fresh buffer, on one filled with anything, and on one another run has used.  For the entries of a sequence the caller
 * drives (begin -> prepare -> step ... -> end; local_sums -> finalize / apply) this holds for the sequence as a whole, which
 * keeps its schedule, prepared batch and accumulators in the workspace from one of its calls to the next.
 * ------------------------------------------------------------------------------------------- */

/* ---------------------------------------------------------------------------------------------
 * Minibatch samplers
 * ------------------------------------------------------------------------------------------- */
/* sample_from_array(key, arange(capacity), n, 0): 10-round Feistel permutation with cycle walking,
 * evaluated at positions 0..n-1 (d3p/util.py:216-301; minibatch.py:231, :289). */
int d3p_feistel_sample(void* stream, const uint32_t* key_dev, uint32_t capacity, uint32_t n,
                       uint32_t* out_idx_dev);

/* Same permutation from explicit round constants rc_dev[30] = rng_suite.random_bits(key, 32, (10, 3))
 * (util.py:240-242), so that any rng_suite (e.g. d3p.random.debug) can drive the sampler. */
int d3p_feistel_from_constants(void* stream, const uint32_t* rc_dev, uint32_t capacity, uint32_t n,
                               uint32_t* out_idx_dev);

/* poisson_sample_idxs + truncate/suppress bookkeeping (d3p/minibatch.py:29-39, :119-124).
 * Element j is selected iff uniform word j <= q.  out_idx_dev[cutoff]: selected indices in
 * descending order, then unselected indices in descending order (stable argsort reversed).
 * out_counts_dev[0] = number selected, [1] = valid count after truncate (suppress=0) or
 * suppress (suppress=1).  Rank r of `world` generates only keystream words of rows
 * [row_lo, row_hi) when those are passed (0, N for a single GPU). */
size_t d3p_poisson_select_workspace(uint32_t N);
int d3p_poisson_select(void* stream, const uint32_t* key_dev, float q, uint32_t N, uint32_t cutoff,
                       int suppress, uint32_t* out_idx_dev, uint32_t* out_counts_dev,
                       void* workspace_dev, size_t workspace_bytes);
/* rng_kind 0: key_dev is a ChaCha state (d3p.random); 1: a threefry key (d3p.random.debug). */
int d3p_poisson_select_rng(void* stream, int rng_kind, const uint32_t* key_dev, float q, uint32_t N,
                           uint32_t cutoff, int suppress, uint32_t* out_idx_dev,
                           uint32_t* out_counts_dev, void* workspace_dev, size_t workspace_bytes);

/* The same for `num_steps` independent draws in one set of launches (the fused run loop prepares 128 steps at
 * once): step t uses the key at keys_dev + t * key_stride_words and writes out_idx_dev + t * idx_stride_words,
 * out_counts_dev + t * counts_stride_words; the workspace is num_steps x d3p_poisson_select_workspace(N). */
int d3p_poisson_select_batch(void* stream, int rng_kind, const uint32_t* keys_dev, size_t key_stride_words,
                             float q, uint32_t N, uint32_t cutoff, int suppress, uint32_t* out_idx_dev,
                             size_t idx_stride_words, uint32_t* out_counts_dev, size_t counts_stride_words,
                             uint32_t num_steps, void* workspace_dev, size_t workspace_bytes);

/* The same selection made by the ranks of a row-sharded data-parallel run, each for the rows [row_lo, row_hi) it holds (SURVEY 8(e);
 * d3p/minibatch.py:29-39: element e's draw is keystream word e whoever generates it, so a rank makes the ChaCha20 blocks of its own
 * rows only -- 1 / world of the work -- and obtains the single-GPU mask bit for bit).  Two calls with an all-gather of the shards'
 * counts between them (d3p_xchg_poisson_counts below; the run loops with the one-shot exchange do all three per prepared batch):
 *   d3p_poisson_shard_flags: the shard's part of the mask and its selected count per step -> shard_counts_dev[t];
 *   d3p_poisson_shard_write: given, per step, counts {selected in the whole table, valid after truncate / suppress
 *     (minibatch.py:119-124)} at counts_dev + t * counts_stride_words and above_dev[t] = selected elements in the shards with HIGHER
 *     rows: the shard's valid selected rows at their GLOBAL batch positions in out_idx (descending row order, :36-37; other entries
 *     are not touched) and its dense list of owned positions (plist_dev, nullable; stride idx_stride_words like out_idx).
 * Same workspace for both (num_steps x d3p_poisson_select_workspace(16 * chunks of the shard) <= that of the whole table).  ABI 7. */
int d3p_poisson_shard_flags(void* stream, int rng_kind, const uint32_t* keys_dev, size_t key_stride_words, float q, uint32_t N,
                            uint32_t row_lo, uint32_t row_hi, uint32_t num_steps, uint32_t* shard_counts_dev, void* workspace_dev,
                            size_t workspace_bytes);
int d3p_poisson_shard_write(void* stream, uint32_t N, uint32_t row_lo, uint32_t row_hi, uint32_t cutoff, const uint32_t* counts_dev,
                            size_t counts_stride_words, const uint32_t* above_dev, uint32_t* out_idx_dev, uint32_t* plist_dev,
                            size_t idx_stride_words, uint32_t num_steps, void* workspace_dev, size_t workspace_bytes);

/* jnp.take(a, idx, axis=0) for a row-major table (minibatch.py:126-129, :210, :233, :306).
 * If valid_count_dev != NULL, output rows >= *valid_count_dev are zero-filled (the mask multiply
 * of minibatch.py:127-129).  row_bytes must be a multiple of 4.  An index >= n_rows is clamped to the last row
 * (jnp.take's "clip"; the samplers never produce one), never dereferenced. */
int d3p_take_rows(void* stream, const void* table_dev, uint64_t n_rows, uint32_t row_bytes,
                  const uint32_t* idx_dev, uint32_t n, const uint32_t* valid_count_dev,
                  void* out_dev);

/* ---------------------------------------------------------------------------------------------
 * DP-VI stages on materialised (B x P) per-example gradients.  The reference's tests call these
 * five stages directly (tests/test_dpsvi.py:128-129, :158-159, :171, :185, :199-202).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t d;         /* feature columns of X */
    int32_t intercept; /* 0/1; latent dimension D = d + intercept; P = 2*D */
    float prior_w;     /* prior std of w   (README.md:93; examples/logistic_regression.py:61) */
    float prior_b;     /* prior std of the intercept (examples/logistic_regression.py:62) */
    float lik_scale;   /* plate scale = num_obs_total (examples/logistic_regression.py:65) */
    float inv_obs;     /* 1 / observation_scale (svi.py:278) */
    /* ABI 2: likelihood family and guide transform.  Zero-initialised tails give the ABI-1 meaning. */
    int32_t family;          /* D3P_FAMILY_LOGREG: ys ~ Bernoulli(logits = xs.w + b)   (README.md:89-99)
                              * D3P_FAMILY_GAUSS_MEAN: obs ~ Normal(mu, lik_sigma).to_event(1), mu ~ Normal(0, prior_w)
                              *   (examples/simple_gaussian_posterior.py:51-65; y_dev unused, intercept must be 0) */
    int32_t guide_transform; /* D3P_GUIDE_SOFTPLUS: scale = softplus(u) (AutoDiagonalNormal);
                              * D3P_GUIDE_EXP: scale = exp(u) (the hand-written guides of the examples,
                              *   examples/simple_gaussian_posterior.py:77-81: mu_loc, mu_std_log);
                              * D3P_GUIDE_EXP_SITES: scale = exp(u), two sample sites and four parameter leaves (the guide of
                              *   examples/logistic_regression.py:67-86, intercept = 1): 'w' and 'intercept' draw their eps from
                              *   their own site keys, the Gaussian mechanism draws one key per leaf, and params / adam_m / adam_v
                              *   are in tree order [intercept_loc, intercept_std_log, w_loc (d), w_std_log (d)].  Accepted by the
                              *   single-GPU runs only (d3p_dpvi_logreg_run, _run_from, _run_particles_from with one particle,
                              *   _run_status); every other entry point refuses it before any launch. */
    float lik_sigma;         /* observation std of D3P_FAMILY_GAUSS_MEAN and D3P_FAMILY_LINREG */
} d3p_logreg_model;

#define D3P_FAMILY_LOGREG 0
#define D3P_FAMILY_GAUSS_MEAN 1
/* Generalised linear models on the logistic regression's kernels (same latent layout, labels required).  They run wherever
 * D3P_FAMILY_GAUSS_MEAN runs, on one GPU: the staged per-example rows, the fused update, d3p_dpvi_logreg_run / _run_from (Feistel
 * and Poisson batches), rows wider than 2048 columns, d3p_logreg_evaluate and the *_particles entries.  Refused with
 * D3P_E_UNSUPPORTED before any launch: a row range that is not the whole table (data-parallel shards) and D3P_GUIDE_EXP_SITES. */
#define D3P_FAMILY_LINREG 2  /* ys ~ Normal(xs.w + b, lik_sigma); lik_sigma finite and > 0 */
#define D3P_FAMILY_POISSON 3 /* ys ~ Poisson(rate = exp(xs.w + b)); labels are counts stored as floats (not checked) */
#define D3P_GUIDE_SOFTPLUS 0
#define D3P_GUIDE_EXP 1
#define D3P_GUIDE_EXP_SITES 2

/* _compute_per_example_gradients for the logistic-regression + AutoDiagonalNormal workload
 * (svi.py:238-308).  params_dev = [auto_loc (D) | auto_scale unconstrained (D)].
 * Noise source: eps_dev (B x D, "parity mode") or, if NULL, generated on chip from the threefry
 * key jax_key_dev exactly as svi.py:289-290 + numpyro's handlers would.
 * mask_dev: B bytes (0/1) or NULL.  Outputs: px_loss_dev[B], px_grads_dev[B x P],
 * meta_dev[0] = num_elements, meta_dev[1] = batch_mask_scaling_factor (svi.py:305). */
size_t d3p_logreg_px_grads_workspace(const d3p_logreg_model* model, uint32_t B);
int d3p_logreg_px_grads(void* stream, const d3p_logreg_model* model, const float* params_dev,
                        const float* X_dev, const float* y_dev, const uint8_t* mask_dev, uint32_t B,
                        const float* eps_dev, const uint32_t* jax_key_dev, float* px_loss_dev,
                        float* px_grads_dev, float* meta_dev, void* workspace_dev,
                        size_t workspace_bytes);

/* DPSVI.evaluate (svi.py:436-449): -ELBO of the batch (B rows) at the current parameters with one guide
 * draw; jax_key_dev = convert_to_jax_rng_key(split(state.rng_key, 1)[0]); model->lik_scale = num_obs_total. */
size_t d3p_logreg_evaluate_workspace(const d3p_logreg_model* model, uint32_t B);
int d3p_logreg_evaluate(void* stream, const d3p_logreg_model* model, const float* params_dev,
                        const float* X_dev, const float* y_dev, uint32_t B, const uint32_t* jax_key_dev,
                        float* loss_dev, void* workspace_dev, size_t workspace_bytes);

/* GaussianMixture(locs, scales, pis).log_prob(x) for B rows of x (d3p/gmm.py:71-86; BASELINE config 3's
 * density).  x: B x d, locs/scales: K x d, pis: K (a simplex; validated by the host layer), K <= 64.
 * Special values follow jax's logsumexp: a row whose every component is -inf (an infinite coordinate, or a finite one so far out
 * that z * z leaves float32) is -inf, not NaN; a row with a NaN component is NaN; pis_k = 0 drops component k. */
int d3p_gmm_log_prob(void* stream, const float* x_dev, uint32_t B, int32_t d, const float* locs_dev,
                     const float* scales_dev, const float* pis_dev, int32_t K, float* out_dev);

/* _compute_per_example_gradients for the Gaussian-mixture MODEL of BASELINE config 3
 * (examples/gaussian_mixture_model.py:51-85: pis ~ Dirichlet(1), mus ~ Normal(0, prior_mu_scale), sigs ~
 * InverseGamma(1, 1), obs ~ GaussianMixture(mus, sigs, pis); guide pis ~ Dirichlet(exp(alpha_log)),
 * mus ~ Normal(mus_loc, 1), sigs ~ InverseGamma(1, 1); svi.py:238-308).
 * params_dev = [alpha_log (K) | mus_loc (K x d)], P = K + K d; one guide draw per example from jax_key_dev
 * (stream layout: oracle/d3p_oracle.c, d3po_gmm_*).  Outputs as d3p_logreg_px_grads; latents_out_dev (optional,
 * B x (K + 2 K d)) receives every example's (gamma draws, eps of mus, sigs).  K <= 16 with d <= 256 or
 * K <= 32 with d <= 128. */
typedef struct {
    int32_t K, d;
    float prior_mu_scale; /* 10 (examples/gaussian_mixture_model.py:65) */
    float lik_scale;      /* plate scale = num_obs_total */
    float inv_obs;        /* 1 / observation_scale (svi.py:278) */
} d3p_gmm_model;

size_t d3p_gmm_px_grads_workspace(int32_t K, uint32_t B);
int d3p_gmm_px_grads(void* stream, const d3p_gmm_model* model, const float* params_dev, const float* X_dev,
                     const uint8_t* mask_dev, uint32_t B, const uint32_t* jax_key_dev, float* px_loss_dev,
                     float* px_grads_dev, float* meta_dev, float* latents_out_dev, void* workspace_dev,
                     size_t workspace_bytes);

/* _clip_gradients: every row scaled by 1/max(1, ||row||_2 / c) in place (svi.py:68-124, :310-325).
 * c == 0 -> D3P_E_INVALID_ARG (the reference raises ValueError, svi.py:119-120). */
int d3p_clip_rows(void* stream, float* px_grads_dev, uint32_t B, uint32_t P, float c);

/* full_norm of a flat vector (svi.py:68-87) -> out_dev[0]. n == 0 gives 0. */
int d3p_full_norm(void* stream, const float* v_dev, uint64_t n, float* out_dev, void* workspace_dev,
                  size_t workspace_bytes);
/* ABI 5: numpy.linalg.norm(v, ord) of the same vector for any order (`ord` of full_norm / normalize_gradient,
 * d3p/svi.py:68-103): 0 = number of non-zero entries, 1, 2 (= d3p_full_norm), +-inf = largest / smallest magnitude, any
 * other p: (sum |x|^p)^(1/p).  n >= 1. */
int d3p_full_norm_ord(void* stream, const float* v_dev, uint64_t n, double ord, float* out_dev);

/* _combine_gradients: column means over the padded batch and mean loss (svi.py:327-348). */
int d3p_combine(void* stream, const float* px_grads_dev, const float* px_loss_dev, uint32_t B,
                uint32_t P, float* avg_dev, float* loss_dev);

/* _perturb_and_reassemble_gradients + perturbation_function (svi.py:350-377, :470-498):
 * out = (avg + normal(site_key) * dp_scale * c / n) * obs_scale * factor with one key per site
 * from split(key, n_sites); meta_dev = {n, factor} as produced above. */
int d3p_perturb(void* stream, const uint32_t* key_dev, const float* avg_dev,
                const int32_t* site_sizes_host, int n_sites, float dp_scale, float c,
                const float* meta_dev, float obs_scale, float* out_dev,
                uint32_t* site_keys_dev /* scratch: n_sites x 16 words */);

/* The same with the standard-normal draws supplied (noise_dev[n], from any rng_suite.normal):
 * out = (avg + noise * dp_scale * c / meta[0]) * obs_scale * meta[1]  (svi.py:365-375, :487-488). */
int d3p_perturb_apply(void* stream, const float* avg_dev, const float* noise_dev, uint64_t n,
                      float dp_scale, float c, const float* meta_dev, float obs_scale, float* out_dev);

/* numpyro.optim.Adam step (svi.py:379-393; examples/logistic_regression.py:141).
 * step_dev: int32 device counter (incremented).  Where g * g leaves float32 the second moment is +inf, as the reference's
 * (1 - b2) * square(g), and the parameter keeps its value. */
int d3p_adam_step(void* stream, float* params_dev, float* m_dev, float* v_dev, int32_t* step_dev,
                  const float* grads_dev, uint32_t P, float lr, float b1, float b2, float eps);

/* numpyro.optim.SGD step (tests/test_dpsvi.py:57): params -= lr * grads; step_dev incremented. */
int d3p_sgd_step(void* stream, float* params_dev, int32_t* step_dev, const float* grads_dev, uint32_t P,
                 float lr);

/* d3p.optimizers.ADADP step (optimizers.py:29-112; Koskela & Honkela's adaptive learning rate): even steps
 * store x_prev / x_stepped and take half a step, odd steps take the second half step, estimate the local error
 * err = ||(x_stepped - x) / max(1, x_stepped)||_2, rescale lr by min(max(sqrt(tol / err), 0.9), 1.1) and, with
 * stability_check, fall back to x_prev when err > tol.  lr_dev: one float; step_dev incremented.
 * Known answers: tests/test_adadp_optimizer.py:66-131. */
size_t d3p_adadp_workspace(void);
int d3p_adadp_step(void* stream, float* params_dev, float* lr_dev, float* x_stepped_dev, float* x_prev_dev,
                   int32_t* step_dev, const float* grads_dev, uint32_t P, float tol, int stability_check,
                   void* workspace_dev, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * Fused DPSVI.update (svi.py:395-434) -- the north-star path.
 * per-example gradient -> joint L2 clip -> sum, X read once, B x P never materialised.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    float clip;      /* clipping_threshold C (svi.py:182) */
    float dp_scale;  /* sigma (svi.py:183) */
    float lr, b1, b2, adam_eps;
} d3p_dpsvi_hyper;

/* Device-resident training state (DPSVIState, svi.py:37-40, plus Adam moments).  All pointers
 * are device addresses owned by the caller. */
typedef struct {
    uint32_t* rng_key;   /* 2 x 16 words: ping-pong ChaCha state keys */
    int32_t key_slot;    /* host value: which of the two slots holds the current key at entry; a
                            call that performs k updates leaves it in slot (key_slot + k) & 1 */
    float* params;       /* P = 2D: [auto_loc | auto_scale unconstrained] */
    float* adam_m;       /* P */
    float* adam_v;       /* P */
    int32_t* step;       /* optimiser step counter i (numpyro _NumPyroOptim state) */
} d3p_dpsvi_state;

/* Where a step's batch comes from. */
#define D3P_BATCH_EXPLICIT 0 /* X/y ARE the batch (B rows), optional mask: DPSVI.update(state, X, y, mask=) */
#define D3P_BATCH_FEISTEL 1  /* subsample_batchify_data get_batch(i, key) fused in (minibatch.py:217-237) */
#define D3P_BATCH_POISSON 2  /* poisson_batchify_data get_batch(i, key) fused in (minibatch.py:103-131) */

typedef struct {
    int32_t kind;            /* D3P_BATCH_* */
    uint32_t B;              /* batch size (FEISTEL), max_batch_size (POISSON), rows (EXPLICIT) */
    float q;                 /* POISSON sampling rate */
    int32_t suppress;        /* POISSON: handle_oversized_batch == "suppress" */
    const uint32_t* batch_key; /* batchifier state key (16 words, device); NULL for EXPLICIT */
    uint32_t* batch_index;   /* device counter i, fold_in(key, i); incremented per step */
    const uint8_t* mask;     /* EXPLICIT only: B bytes or NULL */
    uint64_t n_rows;         /* N: rows of the full (global) table */
    uint64_t row_lo, row_hi; /* rows held by this rank: X_dev/y_dev point at row_lo (0, N on 1 GPU) */
} d3p_batch_source;

size_t d3p_dpvi_logreg_workspace(const d3p_logreg_model* model, const d3p_batch_source* src);

/* Phase 1 (per rank): key schedule, minibatch indices, fused per-example gradient / clip / sum.
 * sums_dev[P + 2] = [sum_i c_i g_i (P) | sum_i masked loss_i | number of valid examples] over
 * the examples whose rows this rank holds.  eps_dev: optional B x D parity-mode noise. */
int d3p_dpvi_logreg_local_sums(void* stream, const d3p_logreg_model* model,
                               const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                               const d3p_batch_source* src, const float* X_dev, const float* y_dev,
                               const float* eps_dev, float* sums_dev, void* workspace_dev,
                               size_t workspace_bytes);

/* Phase 2 (replicated): mean, Gaussian mechanism (noise added ONCE, after any all-reduce of
 * sums_dev), rescale, Adam, advance keys/counters.  loss_dev[0] receives the batch loss
 * (svi.py:342, :306); grad_out_dev (P, optional) the perturbed gradient.  It launches no per-example kernel, so it takes the
 * sums of d3p_dpvi_logreg_local_sums_particles at every width that entry runs. */
int d3p_dpvi_logreg_finalize(void* stream, const d3p_logreg_model* model,
                             const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                             const d3p_batch_source* src, const float* sums_dev, float* loss_dev,
                             float* grad_out_dev, void* workspace_dev, size_t workspace_bytes);

/* Stepwise form of the two phases for the data-parallel loop (d3p_amd/dist.py): the key schedule and
 * the sampler are evaluated for up to 128 steps at once (`prepare`), so that each step only launches
 * the fused kernel + partial reduction (`step_sums`), and -- after the caller's sum-all-reduce of
 * sums_dev -- `step_finalize`.  `t` is the step index inside the prepared batch.
 *   begin -> { prepare(K) -> K x [ step_sums(t) -> all-reduce -> step_finalize(t) ] }* -> end(total steps)
 * `end` stores the key after `steps_done` updates in slot (key_slot + steps_done) & 1. */
int d3p_dpvi_logreg_begin(void* stream, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                          const d3p_dpsvi_state* state, const d3p_batch_source* src,
                          void* workspace_dev, size_t workspace_bytes);
int d3p_dpvi_logreg_prepare(void* stream, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                            const d3p_dpsvi_state* state, const d3p_batch_source* src,
                            uint32_t num_steps, void* workspace_dev, size_t workspace_bytes);
int d3p_dpvi_logreg_step_sums(void* stream, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                              const d3p_dpsvi_state* state, const d3p_batch_source* src, uint32_t t,
                              const float* X_dev, const float* y_dev, const float* eps_dev,
                              float* sums_dev, void* workspace_dev, size_t workspace_bytes);
int d3p_dpvi_logreg_step_finalize(void* stream, const d3p_logreg_model* model,
                                  const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                                  const d3p_batch_source* src, uint32_t t, const float* sums_dev,
                                  float* loss_dev, float* grad_out_dev, void* workspace_dev,
                                  size_t workspace_bytes);
int d3p_dpvi_logreg_end(void* stream, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                        const d3p_dpsvi_state* state, const d3p_batch_source* src,
                        uint32_t steps_done, void* workspace_dev, size_t workspace_bytes);

/* One-launch-per-step form (what d3p_dpvi_logreg_run uses internally), exposed for the data-parallel loop:
 * the cross-workgroup sums of a step live in a 64-bit FIXED-POINT accumulator (integer addition is
 * associative: exact and bitwise reproducible, on one GPU and under any all-reduce order); the update of
 * step g is applied in the prologue of launch g+1.  Accumulator g % 3 of the workspace (layout from
 * d3p_dpvi_logreg_acc_layout: byte offset, int64 words per buffer; three consecutive buffers) is what the
 * caller sum-all-reduces (int64) between launch g and launch g+1.
 *   begin -> acc_reset -> { prepare_buf(K, buf) -> K x [ fused_step(g, t, buf, ...) -> all-reduce(acc[g % 3]) ] }*
 *         -> fused_step(flush_only = 1) -> end(total steps) */
int d3p_dpvi_logreg_prepare_buf(void* stream, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                                const d3p_dpsvi_state* state, const d3p_batch_source* src,
                                uint32_t num_steps, int buf, void* workspace_dev, size_t workspace_bytes);
int d3p_dpvi_logreg_acc_layout(const d3p_logreg_model* model, const d3p_batch_source* src,
                               size_t* offset_bytes, size_t* words_per_buffer);
/* 1 when the model's rows fit the one-launch step (d3p_dpvi_logreg_fused_step), 0 when they run as two-kernel steps (rows too wide for
 * the register-tiled kernel: D > 2048, or D > 1024 unless d % 8 == 0 without intercept): fused_step then returns D3P_E_UNSUPPORTED.  ABI 9. */
int d3p_dpvi_logreg_fused_step_supported(const d3p_logreg_model* model, const d3p_batch_source* src);
int d3p_dpvi_logreg_acc_reset(void* stream, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                              const d3p_dpsvi_state* state, const d3p_batch_source* src,
                              void* workspace_dev, size_t workspace_bytes);
int d3p_dpvi_logreg_fused_step(void* stream, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                               const d3p_dpsvi_state* state, const d3p_batch_source* src, uint32_t g,
                               uint32_t t, int buf, int have_prev, uint32_t prev_t, int prev_buf,
                               const float* X_dev, const float* y_dev, float* prev_loss_dev,
                               int flush_only, void* workspace_dev, size_t workspace_bytes);

/* Single-GPU convenience: `num_steps` x (phase 1 + phase 2) enqueued back to back, i.e. the body of
 * the reference's jit(fori_loop(update)) epoch (examples/logistic_regression.py:149-160).
 * losses_dev: num_steps floats (or NULL). */
int d3p_dpvi_logreg_run(void* stream, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                        const d3p_dpsvi_state* state, const d3p_batch_source* src,
                        const float* X_dev, const float* y_dev, uint32_t num_steps,
                        float* losses_dev, void* workspace_dev, size_t workspace_bytes);

/* The same run as a function of an immutable state (DPSVI.update returns a NEW state, svi.py:395-434; the epoch body of
 * examples/logistic_regression.py:149-160 threads it through fori_loop): it starts from `from` (rng key in slot
 * from->key_slot, optimiser state and step counter; read only) and from batch index `first_batch` (by value;
 * src->batch_index may be NULL) and leaves the result in `state` (state->key_slot must be 0; the final key is in slot
 * num_steps & 1 of state->rng_key).  The state copy and the batch-index word are written by the run's first kernel, so a
 * caller with functional semantics needs no launches of its own around the call.  ABI 4. */
int d3p_dpvi_logreg_run_from(void* stream, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                             const d3p_dpsvi_state* state, const d3p_dpsvi_state* from, const d3p_batch_source* src,
                             uint32_t first_batch, const float* X_dev, const float* y_dev, uint32_t num_steps,
                             float* losses_dev, void* workspace_dev, size_t workspace_bytes);
/* ... and the data-parallel runs d3p_dpvi_logreg_run_dist / d3p_dpvi_logreg_run_xchg (declared below) in the same form:
 * comm (d3p_comm_*: RCCL) or xchg (d3p_xchg_*: one-shot exchange) or neither; the rank's shard is src->row_lo .. row_hi. */
int d3p_dpvi_logreg_run_dist_from(void* stream, void* comm, void* xchg, const d3p_logreg_model* model,
                                  const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state, const d3p_dpsvi_state* from,
                                  const d3p_batch_source* src, uint32_t first_batch, const float* X_dev, const float* y_dev,
                                  uint32_t num_steps, float* losses_dev, void* workspace_dev, size_t workspace_bytes);

/* Times only the dominant kernel (fused gradient/clip/sum) of one step over `reps` launches on
 * `stream` (host out-pointers):
 *   *avg_us       device-side duration: every workgroup stamps the 100 MHz wall clock at entry and
 *                 exit, duration = last exit - first entry (what rocprofv3's kernel trace reports);
 *   *avg_event_us HIP start/stop events recorded around each launch (hipExtLaunchKernel); includes
 *                 the ~4 us dispatch floor an empty kernel also shows (optional, may be NULL).
 * Synchronises the stream; measurement tooling for bench.py, not part of the training path. */
int d3p_dpvi_logreg_time_main_kernel(void* stream, const d3p_logreg_model* model,
                                     const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                                     const d3p_batch_source* src, const float* X_dev,
                                     const float* y_dev, void* workspace_dev, size_t workspace_bytes,
                                     int reps, float* avg_us, float* avg_event_us);

/* DPSVI.evaluate (svi.py:436-449) for the mixture model: -ELBO of the batch with one guide draw;
 * jax_key_dev = convert_to_jax_rng_key(split(state.rng_key, 1)[0]); model->lik_scale = num_obs_total. */
size_t d3p_gmm_evaluate_workspace(const d3p_gmm_model* model, uint32_t B);
int d3p_gmm_evaluate(void* stream, const d3p_gmm_model* model, const float* params_dev, const float* X_dev, uint32_t B,
                     const uint32_t* jax_key_dev, float* loss_dev, void* workspace_dev, size_t workspace_bytes);

/* DPSVI.update (svi.py:395-434) for the mixture model in one call: key split, per-example gradients clipped and
 * summed without materialising B x P, per-site Gaussian noise, numpyro Adam, all enqueued on `stream`.  state as for
 * the logistic-regression path (params = [alpha_log | mus_loc], P = K + K d; the new state key lands in the other
 * key slot).  loss_dev[0]: batch loss; grad_out_dev (P, optional): the perturbed gradient. */
size_t d3p_dpvi_gmm_workspace(const d3p_gmm_model* model, uint32_t B);
int d3p_dpvi_gmm_update(void* stream, const d3p_gmm_model* model, const d3p_dpsvi_hyper* hyper,
                        const d3p_dpsvi_state* state, const float* X_dev, const uint8_t* mask_dev, uint32_t B,
                        float* loss_dev, float* grad_out_dev, void* workspace_dev, size_t workspace_bytes);

/* Data-parallel form of d3p_dpvi_gmm_update, as for the VAE below: a rank holds the B_local examples at positions
 * pos0 .. pos0 + B_local - 1 of the global batch of B_total (the per-example site keys are functions of the GLOBAL position).
 * d3p_dpvi_gmm_local_sums leaves sums_dev[P + 2] = [sum_i c_i g_i | sum_i loss_i | n] of the rank's examples and does not
 * touch the state; the caller sum-all-reduces sums_dev over the ranks; d3p_dpvi_gmm_apply adds the per-site noise once,
 * applies Adam and advances the state identically on every rank.  The workspace is sized for B_local. */
int d3p_dpvi_gmm_local_sums(void* stream, const d3p_gmm_model* model, const d3p_dpsvi_hyper* hyper,
                            const d3p_dpsvi_state* state, const float* X_dev, const uint8_t* mask_dev, uint32_t B_local,
                            uint32_t B_total, uint32_t pos0, float* sums_dev, void* workspace_dev, size_t workspace_bytes);
int d3p_dpvi_gmm_apply(void* stream, const d3p_gmm_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                       float* sums_dev, uint32_t B_total, uint32_t B_local, float* loss_dev, float* grad_out_dev,
                       void* workspace_dev, size_t workspace_bytes);

/* The single-GPU run loop executes the steps of a prepared batch (<= 128) as ONE launch whose workgroups wait on
 * arrival counters for the previous step (bounded waits).  This reads back, after synchronising `stream`, whether any
 * wait of the last run hit its bound (aborted_out != 0: the results of that run are invalid). */
int d3p_dpvi_logreg_chain_status(void* stream, const d3p_logreg_model* model, const d3p_batch_source* src,
                                 void* workspace_dev, size_t workspace_bytes, int32_t* aborted_out);

/* ABI 3: both sticky status words of the last run, after synchronising `stream`.
 *   aborted_out   != 0: a bounded wait of the chained launch ran out; from then on no workgroup applied, published or
 *                       arrived anywhere, i.e. the run stopped advancing -- state and losses of that run are invalid
 *                       (d3p_amd.svi.DPSVI.run_steps raises D3PError).  The value is the code of the FIRST wait that ran
 *                       out: kind | step of its launch << 8 | detail << 20, kinds 1 a wait not told apart, 2 exchange
 *                       workgroup waiting for the step's arrivals, 3 exchange workgroup waiting for the row of rank
 *                       `detail`, 4 compute workgroup waiting for the previous step's release, 5 key-chain link, 6 k_xchg
 *                       waiting for the row of rank `detail` (D3P_ABORT_* in csrc/d3p_logreg_kernel.h;
 *                       d3p_amd._lib.describe_abort turns it into text).  All waits of a launch start with it and run out
 *                       together, so the step names a waiter, not necessarily the place the run stood at; D3P_DBG=64 prints
 *                       the earliest step per kind.
 *   nonfinite_out != 0: a workgroup partial was NaN / Inf or left the fixed-point range of the accumulator; the update that
 *                       followed turned the parameters and the loss into NaN, which is what the reference's float sums
 *                       (svi.py:342-346) give for a diverged model -- never finite garbage. */
int d3p_dpvi_logreg_run_status(void* stream, const d3p_logreg_model* model, const d3p_batch_source* src,
                               void* workspace_dev, size_t workspace_bytes, int32_t* aborted_out, int32_t* nonfinite_out);

/* ABI 8: launch geometry of the chained launch for this model and batch source, without running anything: workgroups per step
 * (0: the shape takes the generic one-launch-per-step kernels) and waves per workgroup, for a single-rank run (data_parallel = 0)
 * or a rank of a data-parallel run with the in-launch exchange (1: src->row_lo / row_hi give its share of the batch).  What the
 * tests use to make sure they cover grids that are NOT a multiple of the 8 XCDs (arrival groups, updaters: DESIGN.md section 6u). */
int d3p_dpvi_logreg_chain_grid(const d3p_logreg_model* model, const d3p_batch_source* src, int data_parallel,
                               uint32_t* workgroups_per_step_out, int32_t* waves_out);

/* Form of the run loops' launches: 0 (default) -- the chained launch where the shape has one: the steps of a prepared batch in
 * ONE launch whose workgroups hand over through arrival counters, which needs the launch's workgroups to make progress
 * together (a GPU shared with other work can starve one: the bounded waits then stop the run, d3p_dpvi_logreg_run_status);
 * 1 -- one launch per step: no cross-workgroup waits at all, ~2 x slower.  DPSVI.run_steps re-runs a stopped run in form 1
 * (the reference's jit(fori_loop) cannot stall; a drop-in must not either).  The switch belongs to the CALLING THREAD and a run
 * reads it once, when it is enqueued: setting it around one run cannot change the form of a run another thread is enqueueing.  ABI 6. */
int d3p_dpvi_logreg_set_run_form(int form);

/* Measurement hook for the run loops (d3p_dpvi_logreg_run, d3p_dpvi_logreg_run_dist): while enabled, every launch of the
 * step kernel is bracketed by HIP start/stop events on the launch stream (hipExtLaunchKernel).
 * d3p_dpvi_logreg_kernel_timing_read synchronises the recorded events, returns the summed kernel time (microseconds), the
 * number of launches and the number of DP-VI steps they covered since the last read, and clears the record.  Process-wide
 * switch, not thread-safe; used by bench.py for the roofline figure of the kernel that runs in the timed region. */
int d3p_dpvi_logreg_kernel_timing_enable(int enable);
int d3p_dpvi_logreg_kernel_timing_read(double* total_us_out, uint32_t* launches_out, uint32_t* steps_out);

/* ---------------------------------------------------------------------------------------------
 * Data-parallel run over the GPUs of one node (the reference is single-device).  One process per GPU;
 * every rank calls the same sequence.  The communicator is RCCL's, created from an id that rank 0 obtains and the
 * host layer distributes (torch.distributed broadcast); librccl.so is resolved at run time.
 * d3p_dpvi_logreg_run_dist = d3p_dpvi_logreg_run on this rank's row shard (src->row_lo / row_hi) with ONE collective
 * per step: the in-place sum-all-reduce of the rank's fixed-point accumulator (4 x (P + 2) int64 words: exact integer
 * sums, so every rank applies bitwise the same update under any reduction order); the Gaussian noise is added once,
 * after the reduce, from the same key on every rank.  comm == NULL runs without the collective.
 * ------------------------------------------------------------------------------------------- */
/* One-shot full-mesh exchange over xGMI (ABI 3; SURVEY 5 / 8e: for a message of 8 KB one hop beats a ring's 2 (n - 1)).
 * Every rank owns an inbox (uncached device memory, double-buffered slots of self-validating words: 32 data bits + the
 * 32-bit tag of the exchange's epoch per 8-byte word, so that a row is its own arrival signal) that its peers map with hipIpc:
 *   d3p_xchg_create   allocates the inbox for messages of `words` int64 words and returns its 80-byte handle (ABI 9: D3P_IPC_HANDLE_BYTES --
 *                     the inbox is a range of ONE hipIpc arena per process, exported once and mapped once by every peer: the handle is
 *                     the arena's 64-byte hipIpc handle + the range's offset + a marker; handle_bytes / handle_stride >= 80);
 *   d3p_xchg_connect  takes the handles of ALL ranks (world x handle_stride bytes, the host layer gathers them, e.g. with
 *                     torch.distributed.all_gather_object) and maps the peers' inboxes;
 *   d3p_xchg_allreduce  enqueues ONE kernel: fold acc_dev[replicas][words] -> write the folded row into slot [rank] of every
 *                     inbox -> poll the n rows of the own inbox until every word carries the epoch's tag -> acc_dev row 0 =
 *                     the sum of the n rows (int64: exact, identical on every rank), rows 1.. = 0.  Every rank must call it
 *                     the same number of times.  Bounded waits (a run stopped by one reports which: D3P_ABORT_* in
 *                     d3p_logreg_kernel.h, handed out as `aborted` by d3p_dpvi_logreg_run_status).
 *   d3p_dpvi_logreg_run_xchg = d3p_dpvi_logreg_run_dist with this exchange as the step's one collective (`words` must be
 *                     the accumulator row of the model: 2 D + 4). */
int d3p_xchg_create(int32_t world, int32_t rank, uint32_t words, void** xchg_out, uint8_t* handle_out, size_t handle_bytes);
int d3p_xchg_connect(void* xchg, const uint8_t* handles, size_t handle_stride);
 /* All-gather of the shards' selected counts of the <= 128 steps of a prepared batch through the exchange's count box (tagged words like
 * the rows; its own epoch), for d3p_poisson_shard_write: per step t counts_dev[t * counts_stride_words + {0, 1}] = {selected in the
 * whole table, valid after truncate (cutoff) / suppress}, above_dev[t] = selected in the shards of the HIGHER ranks (the table is
 * sharded contiguously in rank order), n_owned_dev[t * n_owned_stride_words] = this rank's valid selected rows.  Every rank of the
 * exchange must call it the same number of times.  ABI 7. */
int d3p_xchg_poisson_counts(void* stream, void* xchg, const uint32_t* shard_counts_dev, uint32_t num_steps, uint32_t cutoff, int suppress,
                            uint32_t* counts_dev, size_t counts_stride_words, uint32_t* above_dev, uint32_t* n_owned_dev,
                            size_t n_owned_stride_words);

/* Test / rehearsal helper: the other world - 1 ranks of an exchange played by ONE workgroup on this GPU, enqueued on `stream` (not
 * the stream of the run): for each of the next `num_exchanges` exchanges it waits until this rank's row has arrived in its next
 * peer's inbox and then delivers all-zero rows of every other rank to this rank's inbox.  A run of the 8-rank code paths on one GPU
 * (tests/test_dist.py); the result equals the rank's run with an exchange of its own.  Needs mapped peer inboxes.  ABI 7. */
int d3p_xchg_simulate_peers(void* stream, void* xchg, uint32_t num_exchanges);

/* d3p_xchg_connect_local: the same for ranks that live in ONE process (one stream each): `peers` = the `world` exchange
  * objects of the group, in rank order; their inboxes are wired directly. */
int d3p_xchg_connect_local(void* xchg, void* const* peers, int32_t world);
int d3p_xchg_disconnect(void* xchg);   /* ABI 9: unmap the peers' inboxes; teardown = every rank disconnects -> barrier -> every rank destroys */
int d3p_xchg_destroy(void* xchg);
int d3p_xchg_allreduce(void* stream, void* xchg, long long* acc_dev, int32_t replicas);
int d3p_dpvi_logreg_run_xchg(void* stream, void* xchg, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                             const d3p_dpsvi_state* state, const d3p_batch_source* src, const float* X_dev, const float* y_dev,
                             uint32_t num_steps, float* losses_dev, void* workspace_dev, size_t workspace_bytes);

int d3p_comm_unique_id(uint8_t* id_out, size_t id_bytes); /* id_bytes >= 128 */
int d3p_comm_init(const uint8_t* id, size_t id_bytes, int32_t nranks, int32_t rank, void** comm_out);
int d3p_comm_destroy(void* comm);
int d3p_dpvi_logreg_run_dist(void* stream, void* comm, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                             const d3p_dpsvi_state* state, const d3p_batch_source* src, const float* X_dev,
                             const float* y_dev, uint32_t num_steps, float* losses_dev, void* workspace_dev,
                             size_t workspace_bytes);

/* num_steps x (get_batch(first_batch + t, batch_key) of subsample_batchify_data -> update) on the resident table
 * X_dev (n_rows x d): the body of the example's jit(fori_loop(...)) epoch (examples/gaussian_mixture_model.py:219-230
 * with the subsampling batchifier).  losses_dev[num_steps] optional. */
int d3p_dpvi_gmm_run(void* stream, const d3p_gmm_model* model, const d3p_dpsvi_hyper* hyper,
                     const d3p_dpsvi_state* state, const uint32_t* batch_key_dev, uint32_t first_batch,
                     const float* X_dev, uint32_t n_rows, uint32_t B, uint32_t num_steps, float* losses_dev,
                     void* workspace_dev, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * Variational auto-encoder of BASELINE config 5 (examples/vae.py:65-153) -- the GEMM-shaped model on the path.
 * encoder: h1 = softplus(x W1 + b1), z_loc = h1 Wl + bl, z_std = exp(h1 Ws + bs);  decoder: h2 = softplus(z V1 + c1),
 * obs ~ Bernoulli(sigmoid(h2 V2 + c2)).  Parameter vector = leaves of {'decoder$params', 'encoder$params'} in
 * tree_flatten order: V1 (Z x H), c1 (H), V2 (H x D), c2 (D), W1 (D x H), b1 (H), Wl (H x Z), bl (Z), Ws (H x Z), bs (Z).
 * H2 > 0 (ABI 5): BASELINE config 5's literal 784 -> [400, 200] -> 50 variant, one more dense softplus layer on each side
 * (the reference itself has one hidden layer): encoder x -> H -> H2 -> heads, decoder z -> H2 -> H -> D; leaves
 * V1 (Z x H2), c1, V2 (H2 x H), c2, V3 (H x D), c3, W1 (D x H), b1, W2 (H x H2), b2, Wl (H2 x Z), bl, Ws (H2 x Z), bs
 * (P = 819 284 at 784 / [400, 200] / 50).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t D, H, Z;  /* observation, hidden and latent dimension (784, 400, 50) */
    float scale;      /* scale of every site: plate scale x handlers.scale (vae.py:194-195 -> 1) */
    float inv_obs;    /* 1 / observation_scale (svi.py:278) */
    int32_t H2;       /* width of the second hidden layer; 0 = the reference's one-hidden-layer network */
} d3p_vae_model;

int64_t d3p_vae_num_params(const d3p_vae_model* model);
size_t d3p_dpvi_vae_workspace(const d3p_vae_model* model, uint32_t B);

/* fp32 GEMM on the matrix cores (v_mfma_f32_32x32x2_f32): C[M x N] = alpha * op(A) op(B) (+ bias[n]) (+ C) with element
 * strides A(m, k) = A[m a_sm + k a_sk], B(k, n) = B[k b_sk + n b_sn]; C row-major, leading dimension ldc. */
int d3p_gemm_f32(void* stream, const float* A_dev, int64_t a_sm, int64_t a_sk, const float* B_dev, int64_t b_sk,
                 int64_t b_sn, float* C_dev, int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias_dev,
                 float alpha, int32_t accumulate);

/* ---- test aids (added symbols, ABI 9 unchanged): the options of the VAE's product dispatcher and its grouped launch, reachable
 * on their own so that tests/test_gpu_vae_gemm.py can check every option against a float64 restatement.  Production never calls
 * them.  Both refuse (D3P_E_INVALID_ARG, d3p_last_error) before anything is enqueued whatever the dispatcher cannot run or a
 * product of the VAE step never asks for: null operands an option needs; epilogue 4 or b_row_scale on a product that does not take
 * the bf16 kernel; part_floats < M N (or < force_splits M N); a force_splits the dispatcher's own split choice could not return for
 * this K (the K range rounded up to slices of 32 must reproduce the count and hold two slices or more; at most 16).
 *
 * d3p_gemm_opts mirrors the dispatcher's options (zero = not asked for):
 *   a_last_one    row M - 1 of op(A) is a virtual row of ones: A holds M - 1 rows in memory
 *   part          split-K scratch of part_floats floats ([splits][M][N]); without it a product is never split
 *   epi           0 store; 1 C = softplus(o), C2 = sigmoid(o); 2 C = o * C2; 3 C = [dz | du] with dz = o + ex_sc z,
 *                 du = dz sd eps - ex_sc, [z | sd] = ex_zu (laid out like C, ldc >= 2 N), eps = ex_eps (M x ex_Z dense, ex_Z = N);
 *                 4 (bf16 kernel, k-fast A, n-fast B, unsplit) C = ex_sc (sigmoid(o) - x), x = ep_x laid out like C, and per row and
 *                 group of 32 columns the sums of x o - softplus(o) and of x^2 in ep_ll / ep_xx ([ceil(N / 32)][M])
 *   has_jumps     the displaced segments: columns n >= n_seg of B, bias and C lie b_njump / bias_njump / c_njump elements further,
 *                 rows k >= k_seg of B lie b_kjump further
 *   b_row_scale   (bf16 kernel, n-fast B) row k of B is multiplied by b_row_scale[k] while it is staged
 *   force_splits  K slabs of a product on the bf16 kernel, instead of a count of the dispatcher's own
 *   leave_split   a split product is not reduced: its tiles stay in part and report.splits_left says how many (0: C was written)
 *   exact16_word  caller-owned device word: the entry first enqueues the exactness pass over A with exact16_nonce into it (A
 *                 contiguous, 16-byte aligned, a multiple of 4 elements), then the product reads it: A is taken as exactly
 *                 bf16 iff the word differs from the nonce afterwards
 * d3p_gemm_report: route = the kernel the dispatcher chose (from the variables it branches on), splits = K slabs launched. */
#define D3P_GROUP_MAX 6          /* most products of one grouped launch */
#define D3P_GEMM_ROUTE_F32 0     /* the 64 x 64 kernel; | D3P_GEMM_ROUTE_F32_VA / _VB: 16-byte fetches of A / of B */
#define D3P_GEMM_ROUTE_F32_VA 1
#define D3P_GEMM_ROUTE_F32_VB 2
#define D3P_GEMM_ROUTE_W8 4      /* the eight-wave fp32 kernel (developer switch D3P_GEMM_FP32_MFMA) */
#define D3P_GEMM_ROUTE_BF16X3 5  /* the eight-wave kernel on the bf16 pipe */
#define D3P_GEMM_ROUTE_GROUPED 6 /* appended to a grouped launch */
typedef struct {
    int32_t a_last_one;
    int32_t epi;
    float* part;
    uint64_t part_floats;
    float* C2;
    const float* ex_zu;
    const float* ex_eps;
    const float* ep_x;
    float* ep_ll;
    float* ep_xx;
    int32_t ex_Z;
    float ex_sc;
    int32_t has_jumps, n_seg, k_seg, force_splits;
    int64_t b_njump, b_kjump, bias_njump, c_njump;
    const float* b_row_scale;
    uint32_t* exact16_word;
    uint32_t exact16_nonce;
    int32_t leave_split;
} d3p_gemm_opts;
typedef struct {
    int32_t route, splits, splits_left;
} d3p_gemm_report;
int d3p_gemm_f32_ex(void* stream, const float* A_dev, int64_t a_sm, int64_t a_sk, const float* B_dev, int64_t b_sk,
                    int64_t b_sn, float* C_dev, int32_t ldc, int32_t M, int32_t N, int32_t K, const float* bias_dev,
                    float alpha, int32_t accumulate, const d3p_gemm_opts* opts, d3p_gemm_report* report);
/* Up to D3P_GROUP_MAX + 1 products appended to ONE grouped launch with a common force_splits (every member: leave_split set, no
 * epilogue, its own force_splits 0), then launched.  Per member: report, and joined = 1 when it became part of the group, 0 when
 * the dispatcher launched it alone (the seventh; one whose operand form differs from the group's; one that does not take the bf16
 * kernel).  sum_in_dev / sum_out_dev / sum_n: optional, *sum_out = sum of sum_in[0 .. sum_n) by one more workgroup of the launch. */
typedef struct {
    const float* A;
    int64_t a_sm, a_sk;
    const float* B;
    int64_t b_sk, b_sn;
    float* C;
    const float* bias;
    int32_t ldc, M, N, K;
    float alpha;
    int32_t accumulate;
    d3p_gemm_opts opts;
    d3p_gemm_report report;
    int32_t joined;
} d3p_gemm_member;
int d3p_gemm_f32_group(void* stream, d3p_gemm_member* members, int32_t n, int32_t force_splits, const float* sum_in_dev,
                       float* sum_out_dev, uint32_t sum_n);

/* Stages 1-3 of DPSVI.update fused (svi.py:238-348): sums_dev[P + 2] = [sum_i c_i g_i | sum_i loss_i | n] without ever
 * forming a per-example gradient: norms by ||a d^T||_F = ||a|| ||d||, clipped sums as A^T (diag(c) Delta) GEMMs.
 * eps_dev (B x Z, optional parity-mode noise) or jax_key_dev (per-example threefry keys, svi.py:289-290).
 * norms_dev (B, optional): per-example gradient norms before clipping; px_loss_dev (B, optional). */
int d3p_vae_step_sums(void* stream, const d3p_vae_model* model, const float* params_dev, const float* X_dev,
                      const uint8_t* mask_dev, uint32_t B, const float* eps_dev, const uint32_t* jax_key_dev, float clip,
                      float* sums_dev, float* norms_dev, float* px_loss_dev, void* workspace_dev,
                      size_t workspace_bytes);

/* DPSVI.evaluate (svi.py:436-449) for the VAE: -ELBO of the batch with one guide draw (eps for all B rows from one key,
 * jax_key_dev = convert_to_jax_rng_key(split(state.rng_key, 1)[0]); eps_dev optionally overrides it);
 * model->scale = handlers.scale x num_obs_total / B (the plate scale of the batch), model->inv_obs = 1. */
int d3p_vae_evaluate(void* stream, const d3p_vae_model* model, const float* params_dev, const float* X_dev, uint32_t B,
                     const uint32_t* jax_key_dev, const float* eps_dev, float* loss_dev, void* workspace_dev,
                     size_t workspace_bytes);

/* One DPSVI.update (svi.py:395-434) for the VAE: key split, the fused sums above, one Gaussian-noise key per
 * parameter leaf (svi.py:487-491; 10 leaves, 14 with model->H2 > 0), numpyro Adam; state as for the other models (P = d3p_vae_num_params). */
int d3p_dpvi_vae_update(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper,
                        const d3p_dpsvi_state* state, const float* X_dev, const uint8_t* mask_dev, uint32_t B,
                        const float* eps_dev, float* loss_dev, float* grad_out_dev, void* workspace_dev,
                        size_t workspace_bytes);
/* The same as a function of an immutable state (as d3p_dpvi_logreg_run_from): reads `from`, writes the new state into
 * `state` (key_slot 0; the next key goes to slot 1 of state->rng_key) -- no 3 x P-float state copy per update.  ABI 4. */
int d3p_dpvi_vae_update_from(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper,
                             const d3p_dpsvi_state* state, const d3p_dpsvi_state* from, const float* X_dev,
                             const uint8_t* mask_dev, uint32_t B, const float* eps_dev, float* loss_dev, float* grad_out_dev,
                             void* workspace_dev, size_t workspace_bytes);

/* num_steps x (get_batch(first_batch + t, batch_key) of subsample_batchify_data -> update) on the resident data set
 * X_dev (n_rows x D): the body of the example's jit(lax.fori_loop(...)) epoch (examples/vae.py:227-246).  Per step
 * fold_in, the Feistel indices, the row gather and the update are enqueued back to back; nothing waits for the host.
 * state is advanced in place: its key is read from slot state->key_slot of state->rng_key (2 x 16 words) and ends up
 * in slot (key_slot + num_steps) & 1.  xb_dev: B x D floats (the gathered batch); idx_dev: B + 16 uint32.  ABI 6. */
int d3p_dpvi_vae_run(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                     const uint32_t* batch_key_dev, uint32_t first_batch, const float* X_dev, uint32_t n_rows, uint32_t B,
                     uint32_t num_steps, float* losses_dev, float* xb_dev, uint32_t* idx_dev, void* workspace_dev,
                     size_t workspace_bytes);

/* Data-parallel form of d3p_dpvi_vae_update (BASELINE config 5, "1 vs 8 GPU"): a rank holds the B_local
 * examples at positions pos0 .. pos0 + B_local - 1 of the global batch of B_total (per-example noise keys are functions of
 * the GLOBAL position, svi.py:289-290).  d3p_dpvi_vae_local_sums leaves sums_dev[P + 2] = [sum_i c_i g_i | sum_i loss_i | n]
 * of the rank's examples; the caller sum-all-reduces sums_dev over the ranks (the ONE collective of the step, 2.76 MB at
 * 784/400/50) and every rank calls d3p_dpvi_vae_apply with the reduced sums: noise once per parameter leaf from the same
 * perturbation key on every rank (svi.py:487-491), identical Adam step, new state key in the other key slot -- replicas stay
 * identical without a broadcast.  state is read by both calls and advanced by apply only.  The workspace is sized for
 * B_local.  d3p_dpvi_vae_update is exactly local_sums + apply with one rank. */
int d3p_dpvi_vae_local_sums(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper,
                            const d3p_dpsvi_state* state, const float* X_dev, const uint8_t* mask_dev, uint32_t B_local,
                            uint32_t B_total, uint32_t pos0, const float* eps_dev, float* sums_dev, void* workspace_dev,
                            size_t workspace_bytes);
int d3p_dpvi_vae_apply(void* stream, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper, const d3p_dpsvi_state* state,
                       const float* sums_dev, uint32_t B_total, uint32_t B_local, float* loss_dev, float* grad_out_dev,
                       void* workspace_dev, size_t workspace_bytes);

/* ABI 8: the data-parallel epoch body as ONE call (examples/vae.py:227-246 with the batch sharded by position): num_steps x
 * [d3p_dpvi_vae_local_sums on the RESIDENT shard X_local_dev -> sum-all-reduce of the P + 2 fp32 sums over `comm` (d3p_comm_*:
 * RCCL; NULL = one rank) -> d3p_dpvi_vae_apply], enqueued back to back on `stream`: nothing waits for the host, the state advances
 * in place (its key ends in slot (key_slot + num_steps) & 1 of state->rng_key, as d3p_dpvi_vae_run leaves it), the step's keys
 * are derived once, the Gaussian-mechanism noise is drawn beside the latent kernel and apply is one launch behind the reduce.
 * buckets = 2: the sums travel in two buckets on a second stream, the decoder's leaves while the encoder's weight-gradient products
 * still run (every clipped sum needs the whole backward pass first: only the tail of the step can overlap a reduce); 1: one
 * all-reduce on `stream`; 0: the library's choice.  fmesh (d3p_fmesh_*, below) instead of comm: the full-mesh collective -- by
 * default FUSED with the tile sums in front of it and the update behind it into one launch (k_vae_fmesh_step: the scatter phase reads
 * the split-K partial tiles, the gather phase applies noise + Adam to a column the moment its sum has arrived); buckets = 1 keeps the
 * three launches apart (same results bit for bit).  losses_dev: num_steps floats or NULL. */
int d3p_dpvi_vae_run_dist(void* stream, void* comm, void* fmesh, const d3p_vae_model* model, const d3p_dpsvi_hyper* hyper,
                          const d3p_dpsvi_state* state, const float* X_local_dev, const uint8_t* mask_dev, uint32_t B_local,
                          uint32_t B_total, uint32_t pos0, uint32_t num_steps, float* losses_dev, int32_t buckets,
                          void* workspace_dev, size_t workspace_bytes);

/* ABI 8: full-mesh sum-all-reduce of a float vector over the GPUs of one node -- the collective of the data-parallel VAE step as
 * the survey asks for it (for MB-sized messages on point-to-point xGMI a full-mesh reduce-scatter + all-gather: two
 * hops with every link carrying 1 / world of the vector, where a ring takes 2 (world - 1) dependent hops).  The reference has no
 * collective (single device).  Rank r owns chunk r of the vector: every rank stores its partials of chunk o into rank o's inbox,
 * the owner adds the world's partials in RANK ORDER (every rank then receives bit for bit the same sums) and stores them into every
 * peer's gather inbox.  A float travels as one 8-byte word {fp32 bits | epoch tag}: the data is its own arrival signal, no fence,
 * no flag.  Inboxes are uncached device memory mapped into the peers with hipIpc handles (d3p_fmesh_create -> exchange the 80-byte
 * handles (D3P_IPC_HANDLE_BYTES, as d3p_xchg_create) -> d3p_fmesh_connect; d3p_fmesh_connect_local wires meshes that live in one process).  d3p_fmesh_allreduce: one launch on
 * `stream`, in place, bounded waits; d3p_fmesh_status (after synchronising `stream`): non-zero when a wait ran out -- the vector of
 * that and every later call is then undefined.  d3p_dpvi_vae_run_dist(..., fmesh) uses it instead of RCCL. */
int d3p_fmesh_create(int32_t world, int32_t rank, uint64_t n_floats, void** fmesh_out, uint8_t* handle_out, size_t handle_bytes);
int d3p_fmesh_connect(void* fmesh, const uint8_t* handles, size_t handle_stride);
int d3p_fmesh_connect_local(void* fmesh, void* const* peers, int32_t world);
int d3p_fmesh_set_grid(void* fmesh, int32_t workgroups);   /* workgroups per launch (default 512 = two per CU, ALL resident together; D3P_FMESH_WGS overrides; ranks that share a GPU: fewer) */
int d3p_fmesh_allreduce(void* stream, void* fmesh, float* buf_dev, uint64_t n_floats);
int d3p_fmesh_status(void* stream, void* fmesh, int32_t* stopped_out);
int d3p_fmesh_disconnect(void* fmesh);   /* ABI 9: as d3p_xchg_disconnect */
int d3p_fmesh_destroy(void* fmesh);

/* Self-test of the wave-level sums the step kernels are built on (wave_sum / wave_sum2: DPP adds from inline assembly), taken
 * directly behind divergent branches: in_dev holds 64 floats per wave, out_dev[3 w + {0, 1, 2}] = the sum of wave w's inputs by
 * wave_sum, and the sums of x and 2 x by wave_sum2.  No reference counterpart (jnp.sum); tests/test_gpu_rng.py.  ABI 7. */
int d3p_selftest_wave_sums(void* stream, const float* in_dev, uint32_t n_waves, float* out_dev);

/* Synthetic workload of SURVEY 8(d) / examples/logistic_regression.py:88-104, generated on device:
 * X[r][c] and y[r] are pure functions of (seed, global row, column). */
int d3p_synth_logreg(void* stream, uint32_t seed, uint64_t row0, uint64_t n_rows, int32_t d,
                     float* X_dev, float* y_dev);

/* ABI 9 -- per-example, per-SITE guide noise of a multi-site mean-field guide (the logistic-regression example's own guide,
 * examples/logistic_regression.py:67-86: `sample('w', Normal(w_loc, exp(w_std_log)))` then `sample('intercept', ...)`), replacing what
 * jax.vmap + numpyro's `seed` handler draw inside svi.py:262-290: eps_dev[i] = [normal(site_key_0, (size_0,)) | normal(site_key_1, ...) | ...]
 * for the examples at positions pos0 .. pos0 + B_local - 1 of a batch of B_total; example p's key = split(jax_key, B_total)[p], its guide
 * seed = split(.)[1], the handler advances `rng, site_key = split(rng)` per sample statement (UNPINNED like the rest of numpyro's key
 * plumbing; n_sites = 1 is the stream the fused kernels draw on chip).  site_sizes_host: n_sites <= 8 sizes (a scalar site: 1). */
int d3p_px_eps_sites(void* stream, const uint32_t* jax_key_dev, uint32_t B_total, uint32_t pos0, uint32_t B_local,
                     const int32_t* site_sizes_host, int32_t n_sites, float* eps_dev);

/* ABI 9 -- DPSVI.update (d3p/svi.py:395-434) for a parameter dict with SEVERAL leaves around the fused clipped sums, e.g. the example's own
 * guide (examples/logistic_regression.py:67-86: intercept_loc, intercept_std_log, w_loc, w_std_log), in nine launches:
 *   d3p_dpvi_leaves_begin -> d3p_px_eps_sites -> d3p_dpvi_logreg_local_sums(eps) -> d3p_dpvi_leaves_finalize.
 * The state's parameters / Adam moments are flat in TREE order (the leaves of the dict sorted by name, as jax.tree_util flattens it);
 * col_of_dev[j] = the fused kernels' column ([loc (D) | unconstrained scale (D)], latent elements in site order) of tree element j.
 * begin: (next_key, gradient key, perturbation key) = split(state key, 3) (svi.py:413-415); jax_key = the gradient key's two threefry words
 * (random/__init__.py:149-155); leaf_keys[k] = split(perturbation key, n_leaves)[k] (svi.py:491); params_kernel[col_of[j]] = params_tree[j]. */
int d3p_dpvi_leaves_begin(void* stream, const uint32_t* state_key_dev, int32_t n_leaves, const float* params_tree_dev,
                          const int32_t* col_of_dev, uint32_t P, uint32_t* next_key_dev, uint32_t* jax_key_dev, uint32_t* leaf_keys_dev,
                          float* params_kernel_dev);
/* finalize: sums_dev = [P clipped sums in kernel column order | loss sum | number of valid examples] as d3p_dpvi_logreg_local_sums (or an
 * all-reduce of it) leaves them.  Per tree element j of leaf k: g = (sums[col_of[j]] / B + normal(leaf_keys[k])[e] * dp_scale * clip / n)
 * * obs_scale * (B / n) (svi.py:343-346, :365-375, :487-488), then numpyro's Adam (svi.py:379-393) from (params, m, v, step)_in into the
 * _out arrays (the update is functional, the inputs are not written); loss = (loss sum / B) * obs_scale * B / n (svi.py:342, :306; n = 0: 0, or
 * NaN when a parameter is not finite, as the masked sum gives there).  leaf_sizes_host: n_leaves <= 16 sizes in tree order; grad_out_dev
 * (nullable): the perturbed gradient in tree order. */
int d3p_dpvi_leaves_finalize(void* stream, const d3p_dpsvi_hyper* hyper, const float* sums_dev, const int32_t* col_of_dev,
                             const uint32_t* leaf_keys_dev, const int32_t* leaf_sizes_host, int32_t n_leaves, uint32_t B, float obs_scale,
                             const float* params_in_dev, const float* m_in_dev, const float* v_in_dev, const int32_t* step_in_dev,
                             float* params_out_dev, float* m_out_dev, float* v_out_dev, int32_t* step_out_dev, float* loss_dev,
                             float* grad_out_dev);

/* ABI 9 -- d3p_logreg_evaluate for a guide with several sample sites (the example's own guide: 'w' (d) then 'intercept' (1)): the one
 * guide draw of SVI.evaluate takes every site's eps from its own key, `rng, site_key = split(rng)` per sample statement; params_dev in the
 * kernels' order [loc (D) | unconstrained scale (D)], latent elements in site order.  site_sizes_host = NULL, n_sites = 1: d3p_logreg_evaluate. */
int d3p_logreg_evaluate_sites(void* stream, const d3p_logreg_model* model, const float* params_dev, const float* X_dev,
                              const float* y_dev, uint32_t B, const uint32_t* jax_key_dev, const int32_t* site_sizes_host,
                              int32_t n_sites, float* loss_dev, void* workspace_dev, size_t workspace_bytes);

/* ABI 9 -- measurement aid, not part of the reference's path: a streaming device-to-device copy of `bytes` (multiple of 16, both
 * buffers 16-byte aligned) with `bytes_per_lane` = 16 (float4: the figure quoted as the achievable HBM rate, SURVEY 8(d) "also measure
 * a device-to-device copy peak on the box"), 8 or 4 (to calibrate the FETCH_SIZE / WRITE_SIZE counters per access width). */
int d3p_hbm_copy(void* stream, void* dst_dev, const void* src_dev, uint64_t bytes, int32_t bytes_per_lane);

/* ABI 9 additions -- prior and posterior predictive sampling (d3p/modelling.py:39-223; d3p_amd/modelling.py).  The key plumbing
 * restates numpyro / jax (UNPINNED): draw i of n runs on split(key, n)[i] (multi) or on key itself;
 * posterior: model_key, guide_key = split(draw key); every sample statement that takes a key advances its handler's
 * `rng, site_key = split(rng)`.  Keys are threefry (jax) keys: two uint32 words in device memory. */
#define D3P_PREDICT_SCALE_CONST 0   /* Normal(loc_c, scale_c) (a prior) */
#define D3P_PREDICT_SCALE_GIVEN 1   /* scale_dev as given (AutoDiagonalNormal's auto_scale, already constrained) */
#define D3P_PREDICT_SCALE_EXP 2     /* exp(scale_dev) (the hand-written guides' *_std_log, the VAE encoder's log-scale head) */
typedef struct {
    int32_t size;         /* elements of the site (a scalar site: 1) */
    int32_t offset;       /* column of its first element in a row of latent_dev */
    int32_t chain;        /* 0: the model's seed handler, 1: the guide's (posterior only) */
    int32_t key_index;    /* how many key-taking sample statements precede it under that handler; -1: substituted */
    int32_t scale_kind;   /* D3P_PREDICT_SCALE_* */
    float loc_c, scale_c; /* used where loc_dev / scale_dev are NULL */
    const float* loc_dev;     /* nullable: size elements */
    const float* scale_dev;   /* nullable: size elements */
    const float* value_dev;   /* key_index -1: the substituted value (size elements, the same for every draw) */
} d3p_predict_site;

/* latent_dev[i, offset + e] = loc[e] + normal(site key, (size,))[e] * scale[e] for draw i < n and every site (or the substituted
 * value); obs_keys_dev (nullable): obs_keys[i] = the key of the observation site, key index obs_index under handler obs_chain. */
int d3p_predict_draws(void* stream, const uint32_t* key_dev, uint32_t n, int32_t multi, int32_t posterior, const d3p_predict_site* sites_host,
                      int32_t n_sites, int32_t obs_chain, int32_t obs_index, float* latent_dev, int64_t latent_ld, uint32_t* obs_keys_dev);
/* logistic regression (fused): obs_dev[s, r] = uniform(obs_keys[s], (rows,))[r] < sigmoid(X[r] . latent[s, w_off .. w_off + d) + latent[s, b_col])
 * as int32 (b_col = -1: no intercept), X row-major rows x d; the logits and uniforms never reach memory. */
int d3p_predict_logreg(void* stream, const float* X_dev, uint64_t rows, int32_t d, const float* latent_dev, int64_t latent_ld, int32_t w_off,
                       int32_t b_col, uint32_t n, const uint32_t* obs_keys_dev, int32_t* obs_dev);
/* Gaussian mean: obs_dev[i, r, c] = mu[i, c] + normal(obs_keys[i], (rows, d))[r d + c] * obs_scale */
int d3p_predict_gauss(void* stream, const float* mu_dev, int64_t mu_ld, int32_t d, uint64_t rows, uint32_t n, float obs_scale,
                      const uint32_t* obs_keys_dev, float* obs_dev);
/* VAE (examples/vae.py:65-153): X_dev != NULL -> posterior (encoder over the B images once, z_i ~ Normal(z_loc, exp(z_log_std)) per draw),
 * NULL -> prior (z_i ~ Normal(0, 1), or z_subst_dev (B x Z) for every draw); then the decoder over the n B rows and
 * obs = uniform(obs key, (B, D)) < decoder output.  params_dev: the flat VAE parameter vector (d3p_vae_model's layout; the prior
 * reads the decoder part only).  z_dev: n x B x Z floats, obs_dev: n x B x D int32. */
size_t d3p_predict_vae_workspace(const d3p_vae_model* model, uint32_t B, uint32_t n);
int d3p_predict_vae(void* stream, const d3p_vae_model* model, const float* params_dev, const float* X_dev, uint32_t B, const uint32_t* key_dev,
                    uint32_t n, int32_t multi, const float* z_subst_dev, float* z_dev, int32_t* obs_dev, void* workspace_dev, size_t workspace_bytes);

/* Pointwise log-likelihoods over given posterior draws (numpyro.infer.util.log_likelihood; d3p_amd/infer_util.py); added symbols,
 * ABI 9 and d3p_logreg_model unchanged.  With t[s, r] = X[r] . latent[s, w_off .. w_off + d) + latent[s, b_col] (b_col = -1: no intercept;
 * the layout of d3p_predict_logreg) and ll[s, r] = log p(y_r | t[s, r]) of model->family -- UNSCALED: model->lik_scale and inv_obs are
 * not applied, lik_sigma is (D3P_FAMILY_LINREG) -- in float32, no clamps (Poisson: exp(t) = inf gives -inf):
 *   d3p_loglik_rows   out_dev[s, r] = ll[s, r]                                   (n x rows floats)
 *   d3p_loglik_lppd   out_rows_dev[r] = logsumexp_s ll[s, r] - log n             (rows floats; no n x rows intermediate; a row whose
 *                     every draw is -inf gives -inf; deterministic)
 * D3P_E_UNSUPPORTED before any launch: D3P_FAMILY_GAUSS_MEAN and D3P_GUIDE_EXP_SITES (the guide transform is not read otherwise).
 * D3P_E_INVALID_ARG: a null X / y / latent / out, n < 1, d < 1, b_col >= 0 without model->intercept (or the reverse).  rows == 0: D3P_OK,
 * no launch. */
int d3p_loglik_rows(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows, const float* latent_dev,
                    int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, float* out_dev);
int d3p_loglik_lppd(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows, const float* latent_dev,
                    int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, float* out_rows_dev);

/* Posterior predictive mean and variance of the observed site over given posterior draws (d3p_amd/prediction.py); added symbol, ABI 9
 * and d3p_logreg_model unchanged.  With t[s, r] as above, mu = E[y | t] = sigmoid(t) | t | exp(t) and v = Var[y | t] = mu (1 - mu) |
 * lik_sigma^2 | mu (D3P_FAMILY_LOGREG | LINREG | POISSON):
 *   mean_rows_dev[r] = (1/n) sum_s mu[s, r]
 *   var_rows_dev[r]  = (1/n) sum_s v[s, r] + (1/n) sum_s (mu[s, r] - mean[r])^2        (law of total variance, population form)
 * float32 links without clamps, float64 accumulation in draw order, one rounding to float32; no n x rows intermediate; deterministic.
 * A NaN t makes the row NaN; otherwise a +inf mu (Poisson: exp(t) overflows) makes the row (+inf, +inf), never NaN.  There are no
 * labels.  Arguments, limits and errors are d3p_loglik_lppd's: D3P_E_UNSUPPORTED before any launch for D3P_FAMILY_GAUSS_MEAN and
 * D3P_GUIDE_EXP_SITES; D3P_E_INVALID_ARG for a null X / latent / mean / var, n < 1, d < 1, a latent layout that does not fit, b_col >= 0
 * without model->intercept (or the reverse), a D3P_FAMILY_LINREG lik_sigma that is not finite and > 0; rows == 0: D3P_OK, no launch. */
int d3p_predict_moments(void* stream, const d3p_logreg_model* model, const float* X_dev, uint64_t rows, const float* latent_dev,
                        int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, float* mean_rows_dev, float* var_rows_dev);

/* Predictive sampling of the linear and Poisson regression families (d3p_amd/predictive.py); added symbol, ABI 9 and d3p_logreg_model
 * unchanged.  With t[s, r] as above (d3p_predict_logreg's layout, tile and grid) and obs_keys_dev as d3p_predict_draws returns them:
 *   D3P_FAMILY_LINREG    obs_dev[s, r] = fl(t + fl(normal(obs_keys[s], (rows,))[r] * lik_sigma))        n x rows float32
 *   D3P_FAMILY_POISSON   obs_dev[s, r] = a Poisson(exp(t)) draw by the project's own rule (d3p_predict_glm.hip, DESIGN.md 4b / 4e:
 *                        inversion below a rate of 10, Hoermann's PTRS from there, on the uniforms of fold_in(obs_keys[s], j); NaN t:
 *                        -1, rate 0: 0, rate +inf or a draw above 2^31 - 1: 2147483647)                 n x rows int32
 * t, the normals and the uniforms never reach memory; deterministic.  Arguments, limits and errors are d3p_predict_logreg's, plus:
 * D3P_E_UNSUPPORTED before any launch for every other family and for D3P_GUIDE_EXP_SITES; D3P_E_INVALID_ARG for d != model->d, a
 * D3P_FAMILY_LINREG lik_sigma that is not finite and > 0, b_col >= 0 without model->intercept (or the reverse), and 2 rows >= 2^32 for
 * D3P_FAMILY_POISSON; rows == 0: D3P_OK, no launch. */
int d3p_predict_glm(void* stream, const d3p_logreg_model* model, const float* X_dev, uint64_t rows, int32_t d, const float* latent_dev,
                    int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, const uint32_t* obs_keys_dev, void* obs_dev);

/* Predictive sampling and cluster assignment of the Gaussian mixture model (d3p_amd/mixture.py, d3p_predict_gmm.hip);
 * added symbols, ABI 9 and d3p_gmm_model unchanged.  Limits of all three: k <= 16 with d <= 256 or k <= 32 with d <= 128, otherwise
 * D3P_E_UNSUPPORTED before any launch; k < 1, d < 1, a null required pointer or one not aligned to 4 bytes: D3P_E_INVALID_ARG.
 *
 * d3p_predict_gmm_draws   one launch writes latent_dev, n rows [pis (k) | mus (k d) | sigs (k d)], and obs_keys_dev, n threefry keys.
 *   Draw i runs on split(key, n)[i] (multi == 0: n == 1, the key itself); the prior (posterior == 0) seeds the model's chain with that
 *   key, the posterior splits it into (model, guide); the sites take `chain, site_key = split(chain)` in program order pis, mus, sigs,
 *   then obs on the model's chain.  A site whose *_value_dev is given (prior only) is copied into every draw and takes no key.
 *   pis = g / sum g with g_j the project's own Gamma(alpha_j, 1) draw in float64 (alpha_j = exp(alpha_log_j), prior: 1); mus =
 *   fl(loc + fl(normal scale)) with (loc, scale) = (mus_loc, 1) or (0, prior_mu_scale); sigs = 1 / -logf(u).  n >= 1.
 * d3p_predict_gmm_obs     obs_dev[s, r, c] = fl(mus[z, c] + fl(sigs[z, c] eps)) of draw s's latent row, with component_key, samples_key
 *   = split(obs_keys[s]), z = min(#{j : cum_j < uniform(component_key, (rows, 1))[r]}, k - 1), cum the float32 running sum of pis
 *   left to right, eps = normal(samples_key, (rows, d))[r, c]; zs_out_dev (n x rows int32, nullable) receives z.  latent_ld >= k + 2 k d;
 *   rows d < 2^32, otherwise D3P_E_UNSUPPORTED; n >= 1 (65535 draws per launch, more in several); rows == 0: D3P_OK, no launch.
 * d3p_gmm_assign          a_out_dev[r, j] = log pis_j + sum_c log N(obs[r, c]; mus[j, c], sigs[j, c]) (rows x k float32, nullable) and
 *   argmax_out_dev[r] = argmax_j of that row, the first maximum on ties (rows int32, nullable; a is not written for it); at least one
 *   of the two.  A NaN in a row of a makes the whole row NaN and its argmax -1.  rows d < 2^32; rows == 0: D3P_OK, no launch. */
int d3p_predict_gmm_draws(void* stream, const uint32_t* key_dev, uint32_t n, int32_t multi, int32_t posterior, int32_t k, int32_t d,
                          const float* alpha_log_dev, const float* mus_loc_dev, float prior_mu_scale, const float* pis_value_dev,
                          const float* mus_value_dev, const float* sigs_value_dev, float* latent_dev, uint32_t* obs_keys_dev);
int d3p_predict_gmm_obs(void* stream, const float* latent_dev, int64_t latent_ld, int32_t k, int32_t d, uint64_t rows, uint32_t n,
                        const uint32_t* obs_keys_dev, float* obs_dev, int32_t* zs_out_dev);
int d3p_gmm_assign(void* stream, const float* obs_dev, uint64_t rows, int32_t d, const float* mus_dev, const float* sigs_dev,
                   const float* pis_dev, int32_t k, float* a_out_dev, int32_t* argmax_out_dev);

/* Held-out log predictive density and responsibilities of the Gaussian mixture model over n posterior draws
 * (d3p_amd/mixture_density.py, d3p_gmm_density.hip); added symbols, ABI 9 unchanged.  latent_dev holds n rows
 * [pis (k) | mus (k d) | sigs (k d)] at a leading dimension latent_ld >= k + 2 k d, as d3p_predict_gmm_draws writes them.  With
 *   a[s, r, j] = log pis[s, j] + sum_c log N(obs[r, c]; mus[s, j, c], sigs[s, j, c])            (direct form, float32)
 * d3p_gmm_loglik_rows     ll_out_dev[s, r] = logsumexp_j a[s, r, j]                                               n x rows float32
 * d3p_gmm_loglik_reduce   lppd_out_dev[r] = logsumexp_s ll[s, r] - log n (rows float32, nullable) and resp_out_dev[r, j] = (1 / n)
 *   sum_s exp(a[s, r, j] - ll[s, r]) (rows x k float32, nullable); at least one of the two.  Neither a nor ll reaches memory; obs is
 *   read once; the sums over the draws run in float64 in a fixed order (no atomics, bit-identical between calls).
 * pis[s, j] == 0: the component adds nothing; every component of a draw -inf: ll = -inf (not NaN) and that draw contributes NaN to the
 * row's resp; every draw -inf: lppd = -inf.  A NaN in a row of obs or in a draw's latents makes that row's / that draw's outputs NaN.
 * Limits and errors are d3p_gmm_assign's (k <= 16 with d <= 256 or k <= 32 with d <= 128; rows d < 2^32: D3P_E_UNSUPPORTED), plus
 * 1 <= n <= 2^31 - 1 and latent_ld >= k + 2 k d; every refusal comes before any launch; rows == 0: D3P_OK, no launch. */
int d3p_gmm_loglik_rows(void* stream, const float* obs_dev, uint64_t rows, int32_t d, const float* latent_dev, int64_t latent_ld,
                        int32_t k, uint32_t n, float* ll_out_dev);
int d3p_gmm_loglik_reduce(void* stream, const float* obs_dev, uint64_t rows, int32_t d, const float* latent_dev, int64_t latent_ld,
                          int32_t k, uint32_t n, float* lppd_out_dev, float* resp_out_dev);

/* WAIC (Watanabe-Akaike information criterion; Vehtari, Gelman & Gabry 2017, eqs. 11-13) per row over n posterior draws
 * (d3p_amd/criteria.py); added symbols, ABI 9 unchanged.  With ll[s, r] of d3p_loglik_rows resp. d3p_gmm_loglik_rows:
 *   lppd_rows_dev[r]  = logsumexp_s ll[s, r] - log n              bit-identical to d3p_loglik_lppd's / d3p_gmm_loglik_reduce's value
 *   pwaic_rows_dev[r] = sum_s (ll[s, r] - mean_s ll[s, r])^2 / (n - ddof)       the between-draw variance of ll
 * in one pass, no n x rows intermediate: shifted float64 sums per wave in draw order (the shift is the wave's first finite ll of the
 * row), the waves merged in Chan's pairwise form in a fixed order, one rounding to float32; deterministic.  Every draw of a row equal:
 * pwaic is exactly 0.  A draw with ll = -inf is left out of the sums and makes the row's pwaic +inf (lppd stays finite unless every
 * draw is -inf); a NaN ll makes both outputs of the row NaN; ll = +inf (not reached from finite inputs) makes pwaic NaN.
 * d3p_loglik_waic: arguments, limits and errors are d3p_loglik_lppd's, both outputs required.  d3p_gmm_loglik_waic: those of
 * d3p_gmm_loglik_reduce, both outputs required.  In addition ddof must be 0 or 1 and n > ddof, else D3P_E_INVALID_ARG; rows == 0:
 * D3P_OK, no launch. */
int d3p_loglik_waic(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows, const float* latent_dev,
                    int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, uint32_t ddof, float* lppd_rows_dev, float* pwaic_rows_dev);
int d3p_gmm_loglik_waic(void* stream, const float* obs_dev, uint64_t rows, int32_t d, const float* latent_dev, int64_t latent_ld,
                        int32_t k, uint32_t n, uint32_t ddof, float* lppd_rows_dev, float* pwaic_rows_dev);

/* PSIS-LOO (Pareto-smoothed importance-sampling leave-one-out; Vehtari, Gelman & Gabry 2017, section 2.1 and appendix) per row of a
 * draws x rows log-likelihood matrix (d3p_amd/criteria.py, d3p_psis.hip); added symbol, ABI 9 unchanged.
 * ll_dev[s * ll_ld + r] is the float32 matrix d3p_loglik_rows / d3p_gmm_loglik_rows write; the entry knows nothing of the model.  Per
 * row, in float64 after the loads, one rounding to float32 per output:
 *   x[s] = min_s ll - ll[s]                                    the log importance ratios, the largest shifted to 0
 *   lppd_rows_dev[r] = logsumexp_s ll[s, r] - log n
 *   M = ceil(min(n / 5, 3 sqrt n));  cut = max((M+1)-th largest x, log DBL_MIN);  the tail is the T <= M draws with x > cut (strictly)
 *   the tail, ascending, with e_j = exp(x_j) - exp(cut), is fitted by a generalised Pareto distribution (Zhang & Stephens 2009: m = 30 +
 *   floor(sqrt T) candidates, their profile-likelihood weights, those below 10 DBL_EPSILON dropped); k is regularised to (T k + 5) /
 *   (T + 10) and tail element j is replaced by min(0, log(exp(cut) + sigma expm1(-k log1p(-(j - 0.5) / T)) / k))
 *   elpd_rows_dev[r] = logsumexp_s (x[s] + ll[s]) - logsumexp_s x[s];   k_rows_dev[r] = the regularised k
 * T <= 4 (n = 1 and all draws equal among them), a non-finite k or sigma, or sigma <= 0: the raw ratios stand and k = +inf.  The
 * selection is exact on the float32 values (ties at the cut shorten the tail).  A draw with ll = -inf: elpd = -inf and k = +inf, lppd
 * finite unless every draw is -inf.  A NaN in the column: all three outputs NaN.  ll = +inf: elpd and k NaN, lppd +inf.
 * Deterministic: no floating-point atomics, fixed summation orders, and a row's result does not depend on the other rows of the launch.
 * 1 <= n <= 65535 (M <= 768), ll_ld >= rows, every pointer non-null, aligned to 4 bytes and device memory, else D3P_E_INVALID_ARG
 * before any launch; rows > 32 (2^31 - 1): D3P_E_UNSUPPORTED; rows == 0: D3P_OK, no launch. */
int d3p_psis_loo(void* stream, const float* ll_dev, int64_t ll_ld, uint32_t n, uint64_t rows, float* elpd_rows_dev, float* lppd_rows_dev,
                 float* k_rows_dev);

/* Per-draw sums of the pointwise log-likelihood over a whole table (d3p_amd/diagnostics.py: full-data log joint, ELBO and the Pareto k
 * of a guide's importance ratios; d3p_draw_sums.hip); added symbols, ABI 9 and d3p_logreg_model unchanged.  With ll[s, r]
 * of d3p_loglik_rows, bit for bit (D3P_FAMILY_LOGREG, LINREG and POISSON):
 *   out_draws_dev[s] = sum_{r < rows} ll[s, r]                       n float64; IEEE float64 additions of the float32 values
 * without the n x rows matrix.  Nothing is clamped: a draw with a -inf element (a Poisson rate that overflows float32) gives -inf for
 * that draw only, a NaN gives NaN.  Rows beyond `rows` and draws beyond n contribute nothing.
 * Summation order, fixed (no floating-point atomics; the output bits are identical between calls and a function of the arguments
 * only, not of the device): the table is cut into tiles of 128 rows and those into strips of `per` consecutive tiles,
 *   tiles = ceil(rows / 128);  per = ceil(tiles / 512);  strips = ceil(tiles / per) <= 512          (a function of rows alone)
 * A tile's rows fall into four quarters q = 0..3 of 32 consecutive rows.  For draw s: quarter sum (strip, q) = the elements of quarter
 * q of every tile of the strip, tiles ascending, rows ascending within a tile, added one by one from 0.0; strip partial = ((q0 + q1) +
 * q2) + q3, kept in the workspace as float64 [strip][n]; out[s] = the strips' partials added in ascending strip order from strip 0's,
 * by a second small launch on the same stream.
 * d3p_loglik_draw_sums_workspace(rows, n) = 8 strips n bytes (0 for rows == 0).  Arguments, limits and errors are d3p_loglik_rows' (the
 * same checks in the same order: D3P_E_UNSUPPORTED before any launch for D3P_FAMILY_GAUSS_MEAN and D3P_GUIDE_EXP_SITES;
 * D3P_E_INVALID_ARG for a null X / y / latent / out, n < 1, a latent layout that does not fit, b_col >= 0 without model->intercept or
 * the reverse), then, also before any launch, D3P_E_INVALID_ARG for an out that is not aligned to 8 bytes and for a workspace that is
 * null, not aligned to 8 bytes, not device memory or smaller than the size above.  rows == 0: out is filled with 0.0 (a memset, no
 * launch; the workspace is not read and may be null) and D3P_OK. */
size_t d3p_loglik_draw_sums_workspace(uint64_t rows, uint32_t n);
int d3p_loglik_draw_sums(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows,
                         const float* latent_dev, int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, double* out_draws_dev,
                         void* workspace_dev, size_t workspace_bytes);

/* Per-draw sums of the mixture model's pointwise log-likelihood over a whole table (d3p_amd/mixture_diagnostics.py: full-data log
 * joint, ELBO and the Pareto k of the mixture guide's importance ratios; d3p_gmm_density.hip); added symbols, ABI 9
 * unchanged.  obs and the latents as for d3p_gmm_loglik_rows, and with its ll[s, r] BIT FOR BIT (one kernel text, instantiated for both):
 *   out_dev[s] = sum_{r < rows} ll[s, r]                             n float64; IEEE float64 additions of the float32 values
 * without the n x rows matrix.  Nothing is clamped: a draw with a -inf element (every pis_j of the draw 0) gives -inf for that draw
 * only; a NaN in a row of obs makes every draw NaN, a NaN in a draw's latents that draw only.
 * Summation order, fixed (no floating-point atomics, no arrival order; the output bits are identical between calls, a function of the
 * arguments only and, for draw s, of that draw's latents only): the table is cut into tiles of 64 rows and those into strips of `per`
 * consecutive tiles,
 *   tiles = ceil(rows / 64);  per = ceil(tiles / 2048);  strips = ceil(tiles / per) <= 2048          (a function of rows alone)
 * For draw s: tile sum = the balanced binary tree over the tile's 64 rows in index order, (double)ll of a row below `rows` and exactly
 * 0.0 of a row past it -- level 1 adds rows (0, 1), (2, 3), ..., level 2 those pairs' sums (0..1, 2..3), ..., level 6 the two halves;
 * strip sum = the strip's tile sums added one by one in ascending tile order from 0.0, kept in the workspace as float64 [strip][n];
 * out[s] = the strip sums added in ascending strip order from strip 0's, by a second small launch on the same stream.
 * d3p_gmm_loglik_draw_sums_workspace(rows, d, k, n) = 8 strips n bytes (0 for rows == 0; d and k do not enter).  Arguments, limits and
 * errors are d3p_gmm_loglik_rows' (the same checks in the same order), then, also before any launch, D3P_E_INVALID_ARG for an out that
 * is not aligned to 8 bytes and for a workspace that is null, not aligned to 8 bytes, not device memory or smaller than the size
 * above.  rows == 0: out is filled with 0.0 (a memset, no launch; the workspace is not read and may be null) and D3P_OK. */
size_t d3p_gmm_loglik_draw_sums_workspace(uint64_t rows, int32_t d, int32_t k, uint32_t n);
int d3p_gmm_loglik_draw_sums(void* stream, const float* obs_dev, uint64_t rows, int32_t d, const float* latent_dev, int64_t latent_ld,
                             int32_t k, uint32_t n, double* out_dev, void* workspace_dev, size_t workspace_bytes);

/* Log importance weights of the VAE's guide draws on a held-out batch and per-column float64 statistics (d3p_amd/vae_density.py: the
 * per-image ELBO, the importance-weighted bound on log p(x) and the Pareto k of the amortised guide; d3p_vae_density.hip, DESIGN.md
 * 4l); added symbols, ABI 9 and d3p_vae_model unchanged.  Nothing is scaled: model->scale and model->inv_obs are not read.
 * For draw i < n and image b < B, with (zl_b, zs_b) the encoder's heads at X[b] (zs = the log of the guide's scale) and a_ib the
 * decoder's output pre-activation at z_ib (the passes of d3p_predict_vae through the product kernels):
 *   z_ib       = the z d3p_predict_vae's posterior path draws for (key, n, multi), bit for bit     -> z_out_dev [n][B][Z]
 *   log_px     = sum_c x_bc a_ibc - softplus(a_ibc),   softplus(a) = max(a, 0) + log(1 + exp(-|a|))
 *   log_pz     = sum_j -z^2 / 2 - log(2 pi) / 2
 *   log_qz     = sum_j -u^2 / 2 - zs_bj - log(2 pi) / 2,   u = (z_ibj - zl_bj) exp(-zs_bj)
 *   log_w[i,b] = (log_px + log_pz) - log_qz                                                         -> logw_out_dev [n][B]
 * Every term is float32 arithmetic, each operation rounded on its own; the sums over D and Z are float64 in a fixed order (lane l of a
 * wavefront owns the groups of four consecutive columns g with g mod 64 == l, ascending; Z at lane stride 64; the 64 lane sums merged
 * by the xor butterfly 32, 16, .., 1); log_w is combined in float64 and every output is rounded to float32 once.  parts_out_dev
 * (nullable) receives [3][n][B]: log_px, log_pz, log_qz.  No atomics, no scratch: the output bits are a function of the arguments'
 * values alone -- not of the pointers' alignment (16-byte loads are used where D % 4 == 0 and the rows are aligned, scalar loads
 * otherwise, over the same element-to-lane map) and not of draws_per_slab.
 * The decoder runs over SLABS of whole draws (their z rows are contiguous), so that the workspace holds the activations and logits
 * of one slab only.  The product dispatcher picks its kernel by a product's row count (more than 96 rows: bf16x3), so every slab is
 * kept on the side of that threshold where the call's n B rows fall: n B <= 96 runs as one slab; otherwise a slab has
 * max(draws_per_slab, ceil(97 / B)) draws and a remainder of fewer than ceil(97 / B) draws joins the slab before it.
 * d3p_vae_log_weights_workspace(model, B, draws_per_slab) sizes for the longest such slab, max(draws_per_slab, ceil(97 / B)) +
 * ceil(97 / B) - 1 draws (0 for a bad model, B == 0 or draws_per_slab == 0); n does not enter.
 * Errors, all before any launch: bad model, B == 0, n == 0, n B >= 2^31, B D >= 2^32, B Z >= 2^31, n B Z > 2^40, draws_per_slab == 0, a
 * pointer that is not device memory (parts_out_dev may be null): D3P_E_INVALID_ARG; a workspace below the size above:
 * D3P_E_WORKSPACE.  A NaN in X[b] makes every output of image b NaN and touches no other image. */
size_t d3p_vae_log_weights_workspace(const d3p_vae_model* model, uint32_t B, uint32_t draws_per_slab);
int d3p_vae_log_weights(void* stream, const d3p_vae_model* model, const float* params_dev, const float* X_dev, uint32_t B,
                        const uint32_t* key_dev, uint32_t n, int32_t multi, uint32_t draws_per_slab, float* z_out_dev, float* logw_out_dev,
                        float* parts_out_dev, void* workspace_dev, size_t workspace_bytes);

/* k_vae_logw on its own (tools/time_vae_density.py, tests): the reduction of d3p_vae_log_weights over `rows` rows of given logits
 * [rows][D] and latents z [rows][Z], row r belonging to image r mod B of X [B][D], zl and zs [B][Z]; logw_out_dev [rows],
 * parts_out_dev nullable [3][rows].  The same kernel and the same bits as inside d3p_vae_log_weights.  rows, B, D, Z >= 1, rows < 2^31
 * and device pointers, else D3P_E_INVALID_ARG before the launch. */
int d3p_vae_logw_rows(void* stream, const float* logits_dev, const float* X_dev, const float* z_dev, const float* zl_dev, const float* zs_dev,
                      uint32_t rows, uint32_t B, int32_t D, int32_t Z, float* logw_out_dev, float* parts_out_dev);

/* Per-column statistics of a float32 draws x cols matrix m_dev[s * ld + c] (model-free), in float64 after the loads:
 *   out_dev[0 * cols + c] = mean_s m                          out_dev[1 * cols + c] = sum_s (m - mean)^2 / (n - 1)     (n == 1: NaN)
 *   out_dev[2 * cols + c] = logsumexp_s m - log n             out_dev[3 * cols + c] = (sum_s r)^2 / sum_s r^2,  r = exp(m - max_s m)
 * The draws are cut into four contiguous chunks of ceil(n / 4); each chunk is summed in ascending draw order from 0.0 and the four
 * results are merged as ((c0 + c1) + c2) + c3; two sweeps (sum and max; then the centred squares, sum r and sum r^2); deterministic.
 * A NaN in a column makes its four outputs NaN; every draw -inf: mean = lse = -inf, var = ess = NaN; a +inf draw: lse = +inf, ess = NaN;
 * none of them touches another column.  n >= 1, ld >= cols, m aligned to 4 and out to 8 bytes, both device memory, else
 * D3P_E_INVALID_ARG before any launch; cols >= 2^31: D3P_E_UNSUPPORTED; cols == 0: D3P_OK, no launch. */
int d3p_col_stats(void* stream, const float* m_dev, int64_t ld, uint32_t n, uint64_t cols, double* out_dev);

/* Per-column quantiles of a draws x cols matrix m_dev[s * ld + c] of float32 (dtype 0) or int32 (dtype 1) values (model-free;
 * d3p_amd/intervals.py: credible and predictive intervals; d3p_quantiles.hip); added symbols, ABI 9 unchanged.
 *   out_dev[q * out_ld + c] = the q-th requested quantile of column c, q < Q
 * The HOST turns a probability p into a position, the device does no arithmetic on p: h = (n - 1) p in float64, lo_host[q] = floor(h),
 * g_host[q] = h - lo (p = 1: lo = n - 1, g = 0).  Per column, a = the (lo+1)-th smallest value and b = the (lo+2)-th smallest (b is not
 * read where g == 0), both EXACT on the stored values through an order-preserving uint32 key (float32: -0 taken as +0; int32: the sign
 * bit flipped).  Then in float64: g == 0 or a == b: a; exactly one of a, b infinite (float32 only): that infinity; a = -inf and
 * b = +inf: NaN; otherwise with d = b - a: a + d g where g < 0.5, else b - d (1 - g) -- numpy's method='linear'.  One rounding to
 * float32: an int32 value above 2^24 in magnitude therefore rounds to the nearest float32.  A NaN anywhere in a float32 column makes
 * all Q outputs of that column NaN and touches no other column.
 * Deterministic: no floating-point atomics, and a column's output bits depend on that column's values and on (n, lo, g) alone -- not
 * on ld, out_ld, the other columns of the launch, or on whether the column's keys were staged in LDS (n <=
 * d3p_col_quantiles_staged_max() = 895) or streamed from memory in every pass (n above it).
 * D3P_E_INVALID_ARG before any launch: n outside 1 <= n <= 65535, Q outside 1 <= Q <= 8, a lo >= n, a g outside [0, 1), g != 0 at
 * lo == n - 1, ld < cols, out_ld < cols, a dtype other than 0 / 1, a null pointer, m_dev or out_dev not aligned to 4 bytes or not
 * device memory (lo_host and g_host are HOST memory: Q values each).  cols > 32 (2^31 - 1): D3P_E_UNSUPPORTED; cols == 0: D3P_OK, no
 * launch. */
int d3p_col_quantiles(void* stream, const void* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t cols, uint32_t Q, const uint32_t* lo_host,
                      const double* g_host, float* out_dev, int64_t out_ld);
/* the largest n whose keys d3p_col_quantiles stages in LDS (host only, no device call) */
uint32_t d3p_col_quantiles_staged_max(void);

/* Highest-density intervals per column of a draws x cols matrix m_dev[s * ld + c] of float32 (dtype 0) or int32 (dtype 1) values
 * (model-free; d3p_amd/intervals.py; d3p_hpdi.hip); added symbols, ABI 9 unchanged.  The rule is
 * numpyro.diagnostics.hpdi(x, prob, axis=0), per column of n draws and per window length L = len_host[q] (the HOST computes L =
 * int(prob n), the device does no arithmetic on prob; 0 <= L <= n - 1):
 *   s = the draws sorted ascending;  len[i] = s[i + L] - s[i] for i = 0 .. n - L - 1;  i* = argmin(len), the first minimum;
 *   out_dev[(2 q) * out_ld + c] = s[i*] (the lower end),  out_dev[(2 q + 1) * out_ld + c] = s[i* + L] (the upper end), float32.
 * Both ends are STORED values: no interpolation, and no rounding for float32 input; an int32 count is cast to float32 once (above 2^24
 * in magnitude it rounds to the nearest float32, as d3p_col_quantiles' does).  The order is that of d3p_col_quantiles' uint32 key
 * (float32: -0 taken as +0, so a zero end is +0; int32: the sign bit flipped).  A float32 length is the float32 difference s[i + L] -
 * s[i], one rounding, no contraction -- what numpy computes on a float32 array; an int32 length is the exact integer difference.
 * Ties: the smallest i among the minimal lengths.  A NaN length (inf - inf) is below every other length and the first one wins --
 * np.argmin's rule: [-inf, -inf, 1, 2, inf, inf] gives i* = 0 at every L.  A NaN anywhere in a float32 column makes all 2 Q outputs of
 * that column NaN and touches no other column (the rule of d3p_col_quantiles, not numpy's sort-last).
 * One sort serves all Q lengths.  The column's n keys are sorted in LDS (bitonic network, all-ascending form, exact), one workgroup
 * per d3p_col_hpdi_cols_per_group(n) adjacent columns: 32 (n <= 1152), 8 (n <= 4608), 2 (n <= 18432 = d3p_col_hpdi_max_n()).  There
 * is no streamed form: a larger n is D3P_E_UNSUPPORTED.  Deterministic: no floating-point atomics, no workspace, no host
 * synchronisation; a column's output bits depend on that column's values and on (n, L) alone -- not on ld, out_ld, the other columns
 * of the launch or the form.
 * D3P_E_INVALID_ARG before any launch: n < 1, Q outside 1 <= Q <= 8, a len >= n, ld < cols, out_ld < cols, a dtype other than 0 / 1, a
 * null pointer, m_dev or out_dev not aligned to 4 bytes or not device memory, len_host not host memory (Q values).  n >
 * d3p_col_hpdi_max_n(), or more than 2^31 - 1 column groups: D3P_E_UNSUPPORTED; cols == 0: D3P_OK, no launch. */
int d3p_col_hpdi(void* stream, const void* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t cols, uint32_t Q, const uint32_t* len_host,
                 float* out_dev, int64_t out_ld);
/* the largest n d3p_col_hpdi serves: 18432 (host only, no device call) */
uint32_t d3p_col_hpdi_max_n(void);
/* the columns one workgroup of d3p_col_hpdi owns at n draws: 32, 8, 2, or 0 where n is not served (host only, no device call) */
uint32_t d3p_col_hpdi_cols_per_group(uint32_t n);

/* CRPS and rank (PIT) counts of the draws of every column against an observation (model-free; d3p_amd/scoring.py; d3p_crps.hip, d3p_crps_kernel.h;
 * DESIGN.md 4q); added symbols, ABI 9 unchanged.  m_dev[s * ld + c] is a draws x cols matrix of float32 (dtype 0) or int32 (dtype 1)
 * values, y_dev cols words of the same dtype.  Per column of n draws x_s, sorted ascending as s_0 <= .. <= s_{n-1}, and y = y_dev[c],
 * with d_i = (double)s_i - (double)y, A = sum_i |d_i| and G = sum_i (2 i - n + 1) d_i (= 1/2 sum_i sum_j |x_i - x_j|) in float64:
 *   out_dev[0 * out_ld + c] = crps      = A / n - G / n^2          (the ECDF form: properscoring.crps_ensemble, scoringRules::crps_sample)
 *   out_dev[1 * out_ld + c] = crps_fair = A / n - G / (n (n - 1))  (NaN at n = 1: 0 / 0 is the rule)
 *   out_dev[2 * out_ld + c] = mae       = A / n
 *   out_dev[3 * out_ld + c] = spread    = G / n^2                  (1/2 E|X - X'| over the empirical distribution)
 *   counts_dev[0 * counts_ld + c] = below = #{s : x_s < y},   counts_dev[1 * counts_ld + c] = equal = #{s : x_s == y}
 * each float output rounded to float32 once.  The counts are exact and use IEEE comparison of the values: a NaN draw counts in neither,
 * a NaN y gives 0 and 0, -0 equals +0.  A NaN or +-inf draw, or a non-finite y, makes the column's four float outputs NaN and touches
 * no other column; int32 is never non-finite.  For 0/1 draws crps = (p - y)^2 with p the draws' frequency of 1 (the Brier score).
 * The column is sorted in LDS by d3p_col_hpdi's network, one workgroup per d3p_col_crps_cols_per_group(n) adjacent columns: 32 (n <=
 * 1152), 8 (n <= 4608), 2 (n <= 18432 = d3p_col_crps_max_n()); there is no streamed form: a larger n is D3P_E_UNSUPPORTED.
 * Deterministic: a draw lane adds its terms i = dl, dl + DL, .. in ascending i, the DL = 256 / form lanes of a column merge in one
 * fixed tree; no floating-point atomics, no workspace, no host synchronisation.  A column's output bits depend on that column's
 * values, y and n alone -- not on the order of its draws, ld, out_ld, counts_ld or the other columns of the launch.
 * D3P_E_INVALID_ARG before any launch: a null pointer, a pointer not aligned to 4 bytes, a dtype other than 0 / 1, n < 1, ld < cols,
 * out_ld < cols, counts_ld < cols, m_dev / y_dev / out_dev / counts_dev not device memory.  n > d3p_col_crps_max_n(), or more than
 * 2^31 - 1 column groups: D3P_E_UNSUPPORTED; cols == 0: D3P_OK, no launch. */
int d3p_col_crps(void* stream, const void* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t cols,
                 const void* y_dev,            /* cols words of the matrix's dtype */
                 float* out_dev, int64_t out_ld,        /* 4 rows: crps, crps_fair, mae, spread */
                 uint32_t* counts_dev, int64_t counts_ld /* 2 rows: below, equal */);
/* the largest n d3p_col_crps serves: 18432 (host only, no device call) */
uint32_t d3p_col_crps_max_n(void);
/* the columns one workgroup of d3p_col_crps owns at n draws: 32, 8, 2, or 0 where n is not served (host only, no device call) */
uint32_t d3p_col_crps_cols_per_group(uint32_t n);

/* The conditional mean of the observed site over given posterior draws, as an n x rows matrix (d3p_amd/intervals.py: the matrix
 * d3p_col_quantiles reduces for a credible interval); added symbol, ABI 9 and d3p_logreg_model unchanged.  With t[s, r] as for
 * d3p_loglik_rows:
 *   out_dev[s * out_ld + r] = mu[s, r] = sigmoid(t) | t | exp(t)                       (D3P_FAMILY_LOGREG | LINREG | POISSON)
 * t and the link are formed exactly as d3p_predict_moments forms them (the intercept added as t + latent[s, b_col]; the logistic value
 * from one e = expf(-|t|) as 1 / (1 + e) or e / (1 + e)); float32, no clamps: exp(t) = inf stays inf, a NaN t stays NaN.  Grid and
 * stores are d3p_loglik_rows'.  Arguments, limits and errors are d3p_predict_moments', plus out_ld >= rows (D3P_E_INVALID_ARG):
 * D3P_E_UNSUPPORTED before any launch for D3P_FAMILY_GAUSS_MEAN and D3P_GUIDE_EXP_SITES; rows == 0: D3P_OK, no launch. */
int d3p_predict_mean_rows(void* stream, const d3p_logreg_model* model, const float* X_dev, uint64_t rows, const float* latent_dev,
                          int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, float* out_dev, int64_t out_ld);

/* Per-example gradient norms without the rows (d3p_amd/clipping.py); added symbols, ABI 9 and d3p_logreg_model unchanged.
 *   norms_dev[r] = the float32 L2 norm over all P = 2 D entries of the row d3p_logreg_px_grads writes for example r, r < rows,
 * for the examples at positions pos0 .. pos0 + rows - 1 of ONE batch of B_total examples without a mask: X_dev (rows x d) and y_dev
 * (rows) hold those examples, and the guide draw of example r is eps_r = normal(px_sample_key(jax_key, B_total, pos0 + r), (D,)) --
 * the draw d3p_logreg_px_grads(B = B_total) makes for position pos0 + r -- or row r of eps_dev (rows x D) where that is given.
 * px_loss_dev (nullable, rows): the example's loss as d3p_logreg_px_grads writes it without a mask.  No rows x P tensor exists, in
 * memory or in the workspace (which holds the 5 D derived columns).  The arithmetic is k_logreg_main's; the bits are a function of
 * the arguments (no atomics).  No clamps: a sum of squares beyond float32 gives inf, exp(t) = inf (Poisson) inf or NaN; other rows are
 * unaffected.  Families D3P_FAMILY_LOGREG, _LINREG, _POISSON; guide transforms D3P_GUIDE_SOFTPLUS, _EXP; intercept 0 or 1; d <= 2048.
 * D3P_E_UNSUPPORTED before any launch: D3P_FAMILY_GAUSS_MEAN, D3P_GUIDE_EXP_SITES (pass the sites' eps through eps_dev with
 * D3P_GUIDE_EXP and kernel-order parameters), d > 2048, pos0 + rows > B_total.  rows == 0: D3P_OK, nothing is written. */
size_t d3p_logreg_grad_norms_workspace(const d3p_logreg_model* model, uint32_t rows);
int d3p_logreg_grad_norms(void* stream, const d3p_logreg_model* model, const float* params_dev, const float* X_dev, const float* y_dev,
                          uint32_t B_total, uint32_t pos0, uint32_t rows, const float* eps_dev /* rows x D, or NULL */,
                          const uint32_t* jax_key_dev, float* norms_dev, float* px_loss_dev /* nullable */, void* workspace_dev,
                          size_t workspace_bytes);

/* The profile of a vector of n >= 1 float32 norms against m <= 8 thresholds C_k (finite, > 0) at Q <= 8 quantile positions; added
 * symbols, ABI 9 unchanged.  out_dev receives 29 words of 8 bytes:
 *   [0] n_finite, [1] n_nonfinite (inf or NaN)                                                   uint64
 *   [2] mean, [3] mean of squares, [4] max of the FINITE values (NaN where there is none)         float64
 *   [5 + k]  n_clipped[k]: values > C_k (compared in float32) plus every non-finite one           uint64
 *   [13 + k] mean_clip_factor[k]: the mean over ALL n of min(1, C_k / value) in float64; a non-finite value contributes 0, a value
 *            <= C_k (zero included) 1                                                             float64
 *   [21 + q] the quantile at position q: with the FINITE values sorted, a = the (lo + 1)-th smallest, b = the next one, the result
 *            a + (b - a) g where g < 0.5, else b - (b - a) (1 - g), in float64 on the exactly selected values, rounded to float32 once
 *            and stored as float64 (numpy's method='linear' for lo = floor(h), g = h - lo, h = (n_finite - 1) p, computed by the
 *            CALLER: call once with Q = 0 to learn n_finite).  NaN where lo + 1 (or lo + 2 with g != 0) exceeds n_finite.
 * -0 counts as +0.  The selection is a most-significant-digit radix select over an order-preserving image of the float bits: one pass
 * over the vector per 8-bit digit with all 2 Q ranks in flight, per-workgroup LDS histograms merged with INTEGER atomics; no sort, no
 * n-sized temporary.  The float64 sums are strip partials merged in strip order, the strip count a function of n alone: two calls
 * give identical bits.  thresholds_host, lo_host and g_host are host arrays (g in [0, 1), lo < n); n <= 2^40 (D3P_E_UNSUPPORTED). */
size_t d3p_norm_profile_workspace(uint64_t n);
int d3p_norm_profile(void* stream, const float* norms_dev, uint64_t n, uint32_t m, const float* thresholds_host, uint32_t Q,
                     const uint64_t* lo_host, const double* g_host, void* out_dev, void* workspace_dev, size_t workspace_bytes);

/* Multi-particle ELBO gradients (numpyro Trace_ELBO(num_particles=K)) for the logistic-regression / Gaussian-mean models; added
 * symbols, ABI 9 and d3p_logreg_model unchanged.  For example p of a batch of B with the step's jax key: particle q's key is
 * split(split(jax_key, B)[p], K)[q] (K == 1: split(jax_key, B)[p] itself), the guide draws from it as for one particle.  The
 * example's loss and gradient are the MEANS over its K particles; the mean gradient is what is clipped.  Every entry validates
 * num_particles >= 1 and, at num_particles == 1, is exactly its single-particle counterpart.  K > 1 runs the two-kernel steps
 * (k_logreg_particles + finalize) on one GPU: the data-parallel, chained and persistent forms are not reached. */
/* d3p_logreg_px_grads, averaged over the particles; eps_dev (optional) is B x K x D. */
size_t d3p_logreg_px_grads_particles_workspace(const d3p_logreg_model* model, uint32_t B, uint32_t num_particles);
/* The largest d + intercept that K > 1 runs (host only, no device call): materialising != 0 -> d3p_logreg_px_grads_particles (13630),
 * else d3p_dpvi_logreg_local_sums_particles / d3p_dpvi_logreg_run_particles_from (8178).  Beyond it those entries return
 * D3P_E_UNSUPPORTED before any launch. */
int d3p_logreg_particles_max_latent(int materialising);
int d3p_logreg_px_grads_particles(void* stream, const d3p_logreg_model* model, const float* params_dev, const float* X_dev,
                                  const float* y_dev, const uint8_t* mask_dev, uint32_t B, uint32_t num_particles, const float* eps_dev,
                                  const uint32_t* jax_key_dev, float* px_loss_dev, float* px_grads_dev, float* meta_dev,
                                  void* workspace_dev, size_t workspace_bytes);
/* d3p_dpvi_logreg_local_sums with K particles (eps_dev optional, B x K x D); single GPU (row_lo == 0, row_hi == n_rows). */
int d3p_dpvi_logreg_local_sums_particles(void* stream, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                                         const d3p_dpsvi_state* state, const d3p_batch_source* src, const float* X_dev,
                                         const float* y_dev, const float* eps_dev, uint32_t num_particles, float* sums_dev,
                                         void* workspace_dev, size_t workspace_bytes);
/* d3p_dpvi_logreg_run_from with K particles (explicit batches: DPSVI.update; Feistel / Poisson: the native run_steps loop); the
 * workspace is d3p_dpvi_logreg_workspace's. */
int d3p_dpvi_logreg_run_particles_from(void* stream, const d3p_logreg_model* model, const d3p_dpsvi_hyper* hyper,
                                       const d3p_dpsvi_state* state, const d3p_dpsvi_state* from, const d3p_batch_source* src,
                                       uint32_t first_batch, const float* X_dev, const float* y_dev, uint32_t num_steps,
                                       uint32_t num_particles, float* losses_dev, void* workspace_dev, size_t workspace_bytes);
/* DPSVI.evaluate with K particles: the mean over q of d3p_logreg_evaluate(_sites) at the key split(jax_key, K)[q]. */
size_t d3p_logreg_evaluate_particles_workspace(const d3p_logreg_model* model, uint32_t B, uint32_t num_particles);
int d3p_logreg_evaluate_particles(void* stream, const d3p_logreg_model* model, const float* params_dev, const float* X_dev,
                                  const float* y_dev, uint32_t B, const uint32_t* jax_key_dev, uint32_t num_particles, float* loss_dev,
                                  void* workspace_dev, size_t workspace_bytes);
int d3p_logreg_evaluate_sites_particles(void* stream, const d3p_logreg_model* model, const float* params_dev, const float* X_dev,
                                        const float* y_dev, uint32_t B, const uint32_t* jax_key_dev, const int32_t* site_sizes_host,
                                        int32_t n_sites, uint32_t num_particles, float* loss_dev, void* workspace_dev, size_t workspace_bytes);
/* d3p_px_eps_sites for every particle: eps_dev is B_local x K x (sum of the site sizes). */
int d3p_px_eps_sites_particles(void* stream, const uint32_t* jax_key_dev, uint32_t B_total, uint32_t pos0, uint32_t B_local,
                               uint32_t num_particles, const int32_t* site_sizes_host, int32_t n_sites, float* eps_dev);

/* Model weights for M candidate models from their pointwise elpd vectors (model-free; d3p_amd/model_weights.py; d3p_model_weights.hip;
 * DESIGN.md 4r); added symbols, ABI 9 unchanged.  e_dev[m * ld + r] is a models x rows float32 matrix: row m is model m's pointwise
 * elpd (elpd_loo or elpd_waic), 1 <= M <= 16, 1 <= rows <= 2^32 - 1, ld >= rows; nothing in [rows, ld) is read into a result.  Every
 * value is widened to float64 on load and all arithmetic is float64.  Special values, both entries: a -inf in some models of a row is
 * legitimate (that model's density of the row is 0); a NaN anywhere, a +inf anywhere, or a row that is -inf in every model makes
 * EVERY output NaN.  No floating-point atomics, no cooperative launch, no kernel that waits on another workgroup; the output bits are
 * a function of the arguments alone (not of ld, the device, or what the workspace held).
 * D3P_E_INVALID_ARG before the device is touched: a null pointer, e_dev not aligned to 4 bytes, an output or the workspace not aligned
 * to 8 bytes, M outside 1..16, rows < 1, ld < rows, B outside 1..65535, tol not > 0 (NaN included), max_iter < 1, then pointers that
 * are not device memory; rows > 2^32 - 1: D3P_E_UNSUPPORTED; a workspace shorter than the size function's: D3P_E_WORKSPACE.
 *
 * Stacking of predictive distributions (Yao, Vehtari, Simpson & Gelman 2018): maximise f(w) = sum_r log sum_m w_m exp(e[m, r]) over
 * the simplex by the EM fixed point from w = 1 / M.  With mx_r = max_m e[m, r] and p[m, r] = exp(e[m, r] - mx_r), evaluation j = 0,
 * 1, .. at the current w computes
 *   den_r = sum_k w_k p[k, r] (k ascending),  g_m = (sum_r p[m, r] / den_r) / rows,  f = sum_r (mx_r + log den_r),  gap = max_m g_m - 1
 * and stops with converged = 1 where gap <= tol, with converged = 0 where gap is NaN or j == max_iter; otherwise w_m <- w_m g_m.
 * n_iter = j, the number of updates applied: w_out, gap and f always belong together.  By concavity (f(w*) - f(w)) / rows <= gap.
 * w is not renormalised.  One evaluation is two launches: a strip kernel (the strip count a function of rows alone; a lane adds its
 * rows in ascending order, the 256 lanes merge in one fixed tree) and a one-workgroup kernel that adds the strips' partials in strip
 * order and writes g, gap, f, the new w, the count and a `done` flag to the workspace.  Every launch reads `done` first and returns
 * without writing when it is set.  The host enqueues evaluations in chunks (128; d3p_stacking_set_chunk) and reads the flag once per
 * chunk; the outputs do not depend on the chunk size.  p is recomputed in every evaluation: no rows x M array is written.
 *   w_out_dev: M float64;  info_out_dev: 4 float64 {n_iter, converged, gap, f}. */
size_t d3p_stacking_workspace(uint64_t rows, uint32_t M);
int d3p_stacking_weights(void* stream, const float* e_dev, int64_t ld, uint64_t rows, uint32_t M, double tol, uint32_t max_iter,
                         double* w_out_dev, double* info_out_dev, void* workspace_dev, size_t workspace_bytes);
/* test aid: evaluations enqueued between two reads of the flag; n >= 64, or 0 for the default (128).  Returns the value in force
 * before the call, or -1 (D3P_E_INVALID_ARG) for 0 < n < 64.  Host only, no device call. */
int d3p_stacking_set_chunk(int32_t n);
/* the rows one strip of the stacking kernel covers at least (256: one row per lane); rows / strips grows beyond it (host only) */
uint32_t d3p_stacking_strip_rows(void);

/* Pseudo-BMA+ weights: pseudo-BMA stabilised by the Bayesian bootstrap over the rows, B replicates, 1 <= B <= 65535.  key_dev is a
 * threefry key (2 x uint32, device memory).  Replicate b weighs row r with
 *   g[b, r] = -log(1 - u[b, r]),  u[b, r] = the float32 uniform in [0, 1) of jax.random.uniform's rule applied to
 *   word (r & 1) of threefry2x32(key, (c0, c1) = (r >> 1, b))
 * -- a function of (key, b, r) alone, not of B, rows, ld or the grid.  1 - u is exact in float32; the logarithm is the float64 log of
 * that value.  Per replicate in float64, rows ascending within a strip and strips in ascending order:
 *   S_b = sum_r g[b, r],  T_bm = sum_r g[b, r] e[m, r] (one fused multiply-add per term; a term with g = 0 contributes 0 also where
 *   e = -inf),  z[b, m] = (rows T_bm) / S_b,  w_b = softmax_m z[b, .] (exp(z - max z) over its sum, m ascending)
 *   z_out_dev[b * M + m] = z[b, m];  w_out_dev[m] = (sum_b w_b[m]) / B  (lane t adds b = t, t + 256, .. ascending, one fixed tree)
 * The B x rows matrix is never written: the workspace holds the strips' partials and the B x M replicate weights. */
size_t d3p_bb_pseudo_bma_workspace(uint64_t rows, uint32_t M, uint32_t B);
int d3p_bb_pseudo_bma(void* stream, const uint32_t* key_dev, const float* e_dev, int64_t ld, uint64_t rows, uint32_t M, uint32_t B,
                      double* w_out_dev, double* z_out_dev, void* workspace_dev, size_t workspace_bytes);
/* the rows of one staged chunk of the bootstrap kernel, the least a strip covers (256) (host only, no device call) */
uint32_t d3p_bb_pseudo_bma_strip_rows(void);

/* Per-draw statistics of a replicated data set over its ROWS (d3p_amd/ppc.py: posterior predictive checks; d3p_rep_stats.hip, DESIGN.md
 * 4s); added symbols, ABI 9 and d3p_logreg_model unchanged.  Every other reduction of this library over a draws x rows matrix runs over
 * the draws, once per row; this one runs over the rows, once per draw.
 * For draw s over the values v[s, r], r < rows (float32 or int32, taken to float64 exactly), and a host-given float64 `shift` c, with
 * out_dev of 5 n float64:
 *   out_dev[0 n + s] = sum_r e,  e = fl64(v - c)
 *   out_dev[1 n + s] = sum_r fl64(e e)           the product and the addition are two roundings, never a fused multiply-add
 *   out_dev[2 n + s] = min_r v     out_dev[3 n + s] = max_r v
 *   out_dev[4 n + s] = the number of r with v == 0 (-0.0 counts, NaN does not), an exactly representable float64
 * Summation order of outputs 0 and 1, fixed and exactly d3p_loglik_draw_sums' (no floating-point atomics; the output bits are a function
 * of the arguments only, identical between calls):
 *   tiles = ceil(rows / 128);  per = ceil(tiles / 512);  strips = ceil(tiles / per)                    (a function of rows alone)
 * A tile is four quarters of 32 consecutive rows.  A quarter's accumulator runs over the strip's tiles ascending and rows ascending,
 * starting from 0.0; strip partial = ((q0 + q1) + q2) + q3; the strips are merged in ascending order, starting from strip 0's partial, by
 * a second small launch on the same stream.
 * min and max compare by value; which of +0 / -0 comes back is unspecified.  A NaN anywhere in a draw makes that draw's outputs 0 to 3
 * NaN.  Nothing is clamped.  A draw's result does not depend on the other draws, on ld or on n.  The Poisson family's markers (-1 for a
 * NaN predictor, 2147483647 for saturation) are values like any other: they show up in min and max.
 * Workspace (the contract of "Workspaces": contents on entry unspecified, nothing written outside): d3p_rep_stats_workspace(rows, n) =
 * strips x 5 x n float64 (0 for rows == 0 or rows >= 2^32), shared by both entries.
 *
 * d3p_rep_stats: the model-free form over a matrix that exists, m_dev[s * ld + r], dtype 0 = float32 and 1 = int32 as in
 * d3p_col_quantiles.  Before any launch: D3P_E_INVALID_ARG for a null, misaligned (matrix 4 bytes, out and workspace 8) or non-device
 * pointer, n < 1, rows == 0 (min and max of nothing are undefined), ld < rows, a dtype other than 0 / 1, a non-finite shift or a workspace
 * smaller than the size above; D3P_E_UNSUPPORTED for rows >= 2^32 or n > 128 x 65535.
 *
 * d3p_predict_stats: the fused form, v[s, r] = BIT FOR BIT the outcome d3p_predict_glm (D3P_FAMILY_LINREG: float32, D3P_FAMILY_POISSON:
 * int32) or d3p_predict_logreg (D3P_FAMILY_LOGREG: int32) stores for the same arguments -- the same product tile, intercept add, outcome
 * rule and obs keys -- reduced without the n x rows matrix ever being written.  Arguments, limits and refusals are d3p_predict_glm's for
 * the three families (D3P_E_UNSUPPORTED for D3P_FAMILY_GAUSS_MEAN and D3P_GUIDE_EXP_SITES; D3P_E_INVALID_ARG for d != model->d, a null
 * or non-device X / latent / obs_keys / out, n < 1, a latent layout that does not fit, b_col against model->intercept, Poisson with
 * 2 rows >= 2^32), then rows == 0, an out not aligned to 8 bytes, a non-finite shift and the workspace as above: D3P_E_INVALID_ARG.
 * The outputs equal d3p_rep_stats' of the stored matrix by value, and bit for bit in outputs 0 and 1. */
size_t d3p_rep_stats_workspace(uint64_t rows, uint32_t n);
int d3p_rep_stats(void* stream, const void* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t rows, double shift, double* out_dev,
                  void* workspace_dev, size_t workspace_bytes);
int d3p_predict_stats(void* stream, const d3p_logreg_model* model, const float* X_dev, uint64_t rows, int32_t d, const float* latent_dev,
                      int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n, const uint32_t* obs_keys_dev, double shift,
                      double* out_dev, void* workspace_dev, size_t workspace_bytes);

/* Realized-discrepancy sums of a fitted regression model over its ROWS (d3p_amd/discrepancy.py: the chi-square check of Gelman, Meng &
 * Stern 1996 and the Bayesian R^2; d3p_discrepancy.hip); added symbols, ABI 9 and d3p_logreg_model unchanged.  The one
 * reduction over the rows that needs the observed y, the conditional mean and the replicated outcome together.
 * For draw s and row r, with t the product tile's value (+ the intercept) as in every entry above:
 *   mu = the float32 mean d3p_predict_mean_rows stores for the same arguments (logistic: its two-branch sigmoid; linear: t; Poisson: expf(t))
 *   v  = the outcome d3p_predict_glm / d3p_predict_logreg store for the same arguments, obs keys included (as in d3p_predict_stats)
 * and in float64, every operation rounded once (no fused multiply-add), with the host-given float64 `shift` and sigma = lik_sigma:
 *   M = fl64(mu)     V = fl64(sigma) fl64(sigma) (D3P_FAMILY_LINREG) | M (D3P_FAMILY_POISSON) | M (1.0 - M) (D3P_FAMILY_LOGREG)
 *   q(x) = (e == 0.0) ? 0.0 : (e e) / V,  e = fl64(x) - M          m = M - shift          ey = fl64(y_r) - M
 * out_dev of 6 n float64:
 *   out_dev[0 n + s] = sum_r q(y_r)        the realized discrepancy D(y, theta_s)
 *   out_dev[1 n + s] = sum_r q(v[s, r])    the replicated discrepancy D(y_rep_s, theta_s)
 *   out_dev[2 n + s] = sum_r m             out_dev[3 n + s] = sum_r fl64(m m)
 *   out_dev[4 n + s] = sum_r ey            out_dev[5 n + s] = sum_r fl64(ey ey)
 * ONE convention: a row that is matched exactly (e == 0) contributes nothing, even at V == 0.  Otherwise nothing is clamped: e != 0 at
 * V == 0 gives +inf, a NaN mu gives NaN, and the Poisson family's markers (-1, 2147483647) are values like any other.
 * Summation order of all six: d3p_rep_stats' exactly (tiles, per and strips as above; four quarter accumulators of 32 consecutive rows per
 * tile, tiles and rows ascending from 0.0; strip partial = ((q0 + q1) + q2) + q3; strips merged ascending by a second small launch; no
 * floating-point atomics).  The bits are a function of the arguments alone: a draw's result does not depend on the other draws, on
 * latent_ld or on n.
 * Workspace (the contract of "Workspaces"): d3p_predict_discrepancy_workspace(rows, n) = strips x 6 x n float64 (0 for rows == 0 or
 * rows >= 2^32); its prior content is never read and nothing is written past it.
 * Before any launch, d3p_predict_stats' refusals with y_dev among the pointers (null or non-device: D3P_E_INVALID_ARG), y_dev aligned
 * to 4 bytes, rows == 0, an out not aligned to 8 bytes, a non-finite shift and a short, null, misaligned or non-device workspace:
 * D3P_E_INVALID_ARG; D3P_FAMILY_GAUSS_MEAN and D3P_GUIDE_EXP_SITES: D3P_E_UNSUPPORTED. */
size_t d3p_predict_discrepancy_workspace(uint64_t rows, uint32_t n);
int d3p_predict_discrepancy(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows, int32_t d,
                            const float* latent_dev, int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n,
                            const uint32_t* obs_keys_dev, double shift, double* out_dev, void* workspace_dev, size_t workspace_bytes);

/* Classification metrics of a fitted logistic regression (d3p_amd/classification.py; d3p_classify.hip); added symbols,
 * ABI 9 and d3p_logreg_model unchanged.  Everything below is an INTEGER (counts, pair counts, fixed-point sums): no summation order is
 * promised because none matters, and every output is a function of the arguments alone.
 *
 * d3p_predict_confusion (D3P_FAMILY_LOGREG only; every other family: D3P_E_UNSUPPORTED): for draw s and row r, with t the product
 * tile's value (+ the intercept) as in every entry above,
 *   mu = the float32 mean d3p_predict_mean_rows stores for the same arguments (the two-branch sigmoid)
 *   v  = the 0 / 1 label d3p_predict_logreg stores for the same arguments, obs keys included
 * out_dev of D3P_CONF_COUNTS n uint64, D3P_CONF_COUNTS = 2 + 2 D3P_CONF_THRESHOLDS = 10:
 *   out_dev[0 n + s]           = #{r : (float)v[s, r] == y_r}             (the reference's estimate_accuracy, per draw)
 *   out_dev[1 n + s]           = #{r : mu[s, r] is NaN}
 *   out_dev[(2 + 2 j) n + s]   = #{r : mu[s, r] >= tau[j] and y_r == 1}   true positives at threshold j < T
 *   out_dev[(3 + 2 j) n + s]   = #{r : mu[s, r] >= tau[j] and y_r == 0}   false positives at threshold j < T
 * The comparison is float32 >=: a NaN mu is in neither set, and a NaN threshold counts nothing.  The slots of j >= T are 0.  y_dev: float32
 * labels on the device; a label that is neither 0 nor 1 is in no tp / fp set.  tau_host: T float32 thresholds in HOST memory (read
 * before the entry returns; may be null at T == 0).  The entry zeroes out_dev on the stream and the kernel adds each strip's counts onto
 * it with 64-bit integer atomic adds: no workspace.  d3p_predict_confusion_set_strips(max_strips) (a test aid; 0: the default, 512)
 * changes the grid, never a result.
 * Before any launch, d3p_predict_discrepancy's refusals (model, d, pointers null or not device memory, n, the latent layout, rows == 0,
 * y_dev aligned to 4 bytes, out_dev to 8) and T outside 0..4 or a null tau_host at T > 0: D3P_E_INVALID_ARG; D3P_GUIDE_EXP_SITES and
 * D3P_FAMILY_GAUSS_MEAN / LINREG / POISSON: D3P_E_UNSUPPORTED.
 *
 * d3p_binary_curve: the ROC histogram and the reliability table of one score vector p_dev (float32[rows], probabilities in [0, 1])
 * against labels y_dev (int32[rows] in {0, 1}); model-free.
 *   hist_dev[class][bin] uint32, 2 x D3P_CURVE_BINS, D3P_CURVE_BINS = 0x7E001: with c(x) = float_as_uint(x) >> 12,
 *       bin(p) = c(p) for p < 0.5f,   2 * 0x3F000 - c(1.0f - p) otherwise   (1.0f - p is exact there; -0.0f counts as 0)
 *     a strictly order-preserving map that keeps 11 mantissa bits of min(p, 1 - p) at both ends
 *   calib_dev[3][B] uint64 over B <= 64 equal-width bins, b = min(B - 1, (int)(p * (float)B)) in float32:
 *     calib_dev[0 B + b] = #{r in bin b}   calib_dev[1 B + b] = #{r in bin b, y_r == 1}   calib_dev[2 B + b] = sum_r (uint64)((double)p_r * 2^36)
 *   summary_dev[D3P_CURVE_SUMMARY = 6] uint64: [0] = the rows left out of every table (p NaN, < 0 or > 1, or y outside {0, 1})
 *     [1] = P = the positives   [2] = N = the negatives
 *     [3] = pairs_concordant = sum_b pos_b #{negatives in the bins below b}   [4] = pairs_same_bin = sum_b pos_b neg_b
 *     [5] = max_k |b_k P - a_k N|, a_k / b_k the positives / negatives of the bins 0..k: over P N, the Kolmogorov-Smirnov statistic
 *           max |tpr - fpr| over the bin edges
 * so that (conc + same / 2) / (P N) is the AUC up to the pairs one bin cannot order, and conc / (P N) <= AUC <= (conc + same) / (P N).
 * The entry zeroes the three tables on the stream; equal bins of a wavefront are added once.  rows <= 2^27 (the fixed-point sums stay
 * below 2^63).  Workspace: d3p_binary_curve_workspace() bytes (the per-chunk totals of hist); its prior content is never read.
 * Before any launch: a null, misaligned (p, y, hist: 4 bytes; calib, summary, workspace: 8) or non-device pointer, rows == 0 or
 * > 2^27, B outside 1..64, a short workspace: D3P_E_INVALID_ARG. */
#define D3P_CONF_THRESHOLDS 4
#define D3P_CONF_COUNTS (2 + 2 * D3P_CONF_THRESHOLDS)
#define D3P_CURVE_BINS 0x7E001
#define D3P_CURVE_SUMMARY 6
int d3p_predict_confusion_set_strips(int32_t max_strips);
int d3p_predict_confusion(void* stream, const d3p_logreg_model* model, const float* X_dev, const float* y_dev, uint64_t rows, int32_t d,
                          const float* latent_dev, int64_t latent_ld, int32_t w_off, int32_t b_col, uint32_t n,
                          const uint32_t* obs_keys_dev, const float* tau_host, int32_t T, uint64_t* out_dev);
size_t d3p_binary_curve_workspace(void);
int d3p_binary_curve(void* stream, const float* p_dev, const int32_t* y_dev, uint64_t rows, uint32_t B, uint32_t* hist_dev, uint64_t* calib_dev,
                     uint64_t* summary_dev, void* workspace_dev, size_t workspace_bytes);

/* The energy score of multivariate predictive draws against the observed outcomes (model-free; d3p_amd/energy.py; d3p_energy.hip;
 * DESIGN.md 4v); added symbols, ABI 9 unchanged.  ES = E|X - y| - 1/2 E|X - X'| (Gneiting & Raftery 2007), the multivariate CRPS.
 * draws_dev[s * ld_draw + r * ld_row + c] is draw s < n of row r < rows in column c < d (column stride 1), float32 (dtype 0) or int32
 * (dtype 1: converted to float32 when staged, which is exact for |v| <= 2^24; the Python layer refuses larger magnitudes);
 * y_dev[r * y_ld + c] the observation, of the same dtype.  For row r the items are z_0 .. z_{n-1} (the draws) and z_n = y_r; per pair
 *   t_c = fl32(a_c - b_c),  q = the float32 fmaf chain over c ascending from 0,  dist = the native root of q, widened to float64
 * (1 ulp, exact on perfect squares; the bound of tests/energy_ref.bound carries it; d3p_pair_stats below takes the IEEE root)
 * and with S1 = sum_i dist(z_i, y), S2 = sum_{i != j} dist(z_i, z_j) in float64 in the fixed order d3p_energy.hip states (each
 * unordered pair computed once, counted twice):
 *   out_dev[0 * out_ld + r] = es      = mae - spread
 *   out_dev[1 * out_ld + r] = es_fair = mae - S2 / (2 n (n - 1))   (NaN at n = 1: 0 / 0 is the rule)
 *   out_dev[2 * out_ld + r] = mae     = S1 / n
 *   out_dev[3 * out_ld + r] = spread  = S2 / (2 n^2)
 * each rounded to float32 once.  A NaN or +-inf element among a row's draws or in its y makes that row's four outputs NaN and touches
 * no other row; finite elements whose t_c or q overflows float32 follow IEEE from there (dist = inf).  At d = 1 es is the CRPS of
 * d3p_col_crps up to the two rules' rounding.
 * Two forms, which agree bit for bit: 1, rows (one wavefront per row, d3p_energy_score_rows_per_group(1) = 16 adjacent rows per
 * workgroup) and 2, streamed (one row per workgroup, its pair tiles dealt to four wavefronts).  Both walk pair tiles of
 * d3p_energy_score_tile_draws() = 32 items a side in column chunks of d3p_energy_score_chunk_cols() = 32 staged in LDS, so neither n nor
 * d is bounded by LDS.  d3p_energy_score_form(n, rows, d) is the form the entry takes (0: n or d not served);
 * d3p_energy_score_set_form(form) (a test aid; 0: the rule) forces one and changes no result.
 * Deterministic: no floating-point atomics, no workspace, no host synchronisation; a row's output bits depend on that row's values, y,
 * n and d alone -- not on rows, the other rows, ld_draw, ld_row, y_ld, out_ld, the row's position in a workgroup or the form.
 * D3P_E_INVALID_ARG before any launch: a null pointer, a pointer not aligned to 4 bytes, a dtype other than 0 / 1, n < 1, d < 1,
 * ld_row < d, ld_draw < rows * ld_row, y_ld < d, out_ld < rows, draws_dev / y_dev / out_dev not device memory.  n >
 * d3p_energy_score_max_n() = 65535, or more than 2^31 - 1 workgroups: D3P_E_UNSUPPORTED; rows == 0: D3P_OK, no launch. */
int d3p_energy_score(void* stream, const void* draws_dev, int32_t dtype, int64_t ld_draw, int64_t ld_row, uint32_t n, uint64_t rows, uint32_t d,
                     const void* y_dev, int64_t y_ld,          /* rows x d words of the draws' dtype */
                     float* out_dev, int64_t out_ld            /* 4 rows: es, es_fair, mae, spread */);
/* host only, no device call: the largest n served; the items a side of a pair tile (T); the columns of a staged chunk (C); the rows
 * one workgroup owns in form 1 / 2 (0: no such form); the form taken at a shape */
uint32_t d3p_energy_score_max_n(void);
uint32_t d3p_energy_score_tile_draws(void);
uint32_t d3p_energy_score_chunk_cols(void);
uint32_t d3p_energy_score_rows_per_group(int32_t form);
uint32_t d3p_energy_score_form(uint32_t n, uint64_t rows, uint32_t d);
int d3p_energy_score_set_form(int32_t form);

/* Pair statistics of two tables (model-free; d3p_amd/fidelity.py; d3p_pair_stats.hip); added symbols, ABI 9 unchanged.
 * What the two-sample energy distance (Szekely & Rizzo), the distance to the closest record and the nearest-neighbour adversarial
 * accuracy (Yale et al. 2020) of a synthetic table reduce: ONE O(na nb d) walk over the pairs of two tables.
 * a_dev[i * a_ld + c] is row i < na of the first table in column c < d (column stride 1), b_dev[j * b_ld + c] row j < nb of the second,
 * both float32 (dtype 0) or both int32 (dtype 1: converted to float32 when staged, which is exact for |v| <= 2^24; the Python layer
 * refuses larger magnitudes).  Per pair, d3p_energy_score's chain (both walk the tile of d3p_pair_tile.h) and the IEEE root:
 *   t_c = fl32(a_c - b_c),  q = the float32 fmaf chain over c ascending from 0,  dist = sqrtf(q) correctly rounded
 * never a Gram matrix.  For row i over the admissible j -- all j < nb, without j == i when exclude_diagonal is 1 (na == nb required);
 * duplicate rows are pairs like any other --
 *   sum_dev[i]    = sum_j (double)dist(i, j)   in float64, in the fixed order d3p_pair_stats.hip states, not rounded further
 *   min_dev[i]    = sqrtf(q_min), q_min the smallest q
 *   argmin_dev[i] = the SMALLEST j whose q equals q_min (the tie rule is on q, not on the rounded root)
 * min and argmin are one unsigned 64-bit minimum of (bits(q) << 32) | j: no order to promise.  No admissible j (nb == 1 with the
 * diagonal excluded): sum = 0, min = +inf, argmin = 0xFFFFFFFF.  A NaN or +-inf element in row i of a makes that row's outputs NaN,
 * NaN, 0xFFFFFFFF and touches no other row; one anywhere in b does the same to every row (flags taken while staging, never inf - inf);
 * finite elements whose t_c or q overflows float32 follow IEEE from there (dist = inf, ties at inf to the smallest j).
 * THE ORDER of a row's sum: the rows of b in tiles of d3p_pair_stats_tile_rows() = 32, the tiles in segments of
 * d3p_pair_stats_segment_tiles() = 16, tile J of a segment in slot J mod 4; per slot a lane adds its pairs in ascending J, kj fastest,
 * the 8 lanes of a row meet by the xor butterfly 4, 2, 1; per segment the four slot sums are added in ascending order onto 0, then the
 * segments in ascending order onto 0.  Two forms over that one order, which agree bit for bit: 1, wide (one workgroup per tile of a
 * walks every segment; no workspace) and 2, split (one workgroup per tile of a and segment of b writes a float64 sum, a packed minimum
 * and a flag word per (segment, row) to ws_dev; a second launch adds them in segment order).  d3p_pair_stats_form(na, nb, d) is the form
 * the entry takes (0: a zero argument): split where the tiles of a alone cannot fill the chip; d3p_pair_stats_set_form(form) (a test
 * aid; 0: the rule) forces one and changes no result.  d3p_pair_stats_workspace(na, nb, d) is the size that form needs: 0 for the wide
 * form, where a null ws_dev is fine.  Columns are staged in chunks of d3p_pair_stats_chunk_cols() = 32 in LDS: neither table's length
 * nor d is bounded by it.
 * Deterministic: no floating-point atomics, no host synchronisation; repeated calls give equal bits; a row's three outputs depend on that
 * row's values, b, nb, d and the flag alone -- not on na, the other rows of a, a_ld, b_ld, the row's place in its tile, the form or the
 * workspace's previous contents.
 * Checked before any launch, in this order: a null a_dev / b_dev / sum_dev / min_dev / argmin_dev, a pointer not aligned to 4 bytes
 * (sum_dev, ws_dev: 8), a dtype other than 0 / 1, na < 1, nb < 1, d < 1, a_ld < d, b_ld < d, exclude_diagonal other than 0 / 1 or set with
 * na != nb: D3P_E_INVALID_ARG; ws_bytes below d3p_pair_stats_workspace (or a null ws_dev where it is not 0): D3P_E_WORKSPACE; more than
 * 2^31 - 1 workgroups: D3P_E_UNSUPPORTED; last, a table, an output or a needed workspace that is not device memory:
 * D3P_E_INVALID_ARG. */
int d3p_pair_stats(void* stream, const void* a_dev, const void* b_dev, int32_t dtype, int64_t a_ld, int64_t b_ld, uint32_t na, uint32_t nb,
                   uint32_t d, int32_t exclude_diagonal,
                   double* sum_dev, float* min_dev, uint32_t* argmin_dev,      /* na each */
                   void* ws_dev, size_t ws_bytes);
/* host only, no device call: the rows a side of a pair tile (T); the columns of a staged chunk (C); the tiles of b per segment (G); the
 * form taken at a shape; the workspace that form needs */
uint32_t d3p_pair_stats_tile_rows(void);
uint32_t d3p_pair_stats_chunk_cols(void);
uint32_t d3p_pair_stats_segment_tiles(void);
uint32_t d3p_pair_stats_form(uint32_t na, uint32_t nb, uint32_t d);
size_t d3p_pair_stats_workspace(uint32_t na, uint32_t nb, uint32_t d);
int d3p_pair_stats_set_form(int32_t form);

/* Binned one- and two-way marginal counts of a table (model-free; d3p_amd/marginals.py; d3p_marginals.hip); added symbols,
 * ABI 9 unchanged.  What the total variation distance of the 1- and 2-way marginals and the pairwise association (Cramer's V) of a
 * synthetic table against the real one reduce: per column the histogram of its discretised values, per pair of columns i < j their
 * contingency table, in n d(d - 1)/2 integer increments -- never a one-hot matrix, never a launch per pair.
 * x_dev[r * ld + c] is row r < n in column c < d (column stride 1), float32 (dtype 0) or int32 (dtype 1: converted to float32 when
 * staged, which is exact for |v| <= 2^24; the Python layer refuses larger magnitudes).  Column c has nb_c = nbins_dev[c] bins, 1 <= nb_c
 * <= B, cut by m = nb_c - 1 finite, non-decreasing float32 edges e_k = edges_dev[c * (B - 1) + k], k < m (a d x (B - 1) array; at B = 1
 * it is never read, but the pointer must still be device memory); B <= d3p_marginals_max_bins() = 32.
 * THE CODE of a value v in column c: B, the MISSING cell, if v is NaN; otherwise #{k < m : e_k < v}, numpy's searchsorted(e, v,
 * side="left"): the bins are right-closed, bin 0 holds everything <= e_0 (-inf included), the last bin everything above e_{m-1} (+inf
 * included), and -0.0 and 0.0 are equal.  THE CELL STRIDE is K = B + 1.  Both outputs are uint32 (n <= 2^32 - 1 fits):
 *   one_way_dev[c * K + u]           = the number of rows whose code in column c is u
 *   two_way_dev[(p * K + u) * K + v] = the number of rows with code u in column i and code v in column j, for every pair i < j at the
 *                                      lexicographic index p = i (2 d - i - 1) / 2 + (j - i - 1)
 * The entry zeroes both outputs itself; d = 1 has no pairs (two_way_dev may then be null).  The outputs are integers: a function of the
 * arguments alone, whatever the grid or the order of the atomic adds, and not of ld or of what the workspace held.
 * SAFETY: nbins_dev and edges_dev are device memory the entry cannot read, so the kernel clamps nb_c into [1, B] and searches at most
 * B - 1 entries of column c's own slots: every code lies in [0, B] by construction, whatever those arrays hold (unsorted edges give an
 * unspecified but in-range code).
 * Two launches: the first writes the uint8 code of every element to ws_dev (column-major, n * d bytes = d3p_marginals_workspace(n, d, B);
 * every byte read is written in the same call) and adds the one-way counts, a workgroup owning d3p_marginals_code_rows() = 4096 rows of
 * up to 64 columns; the second gives a workgroup d3p_marginals_pair_tile() = 4 consecutive pairs and a strip of
 * d3p_marginals_strip_rows() = 32768 rows, counts into replicated uint32 LDS histograms (a lane chooses its replica, which spreads the
 * lanes that meet on one cell of a skewed column) and adds the strip's non-zero cells to two_way_dev with integer atomicAdd.  No
 * floating-point atomics, no scratch, no dynamic LDS, no host synchronisation.
 * Checked before any launch, in this order: a null x_dev / nbins_dev / edges_dev / one_way_dev (and two_way_dev where d > 1), a
 * pointer not aligned to 4 bytes, a dtype other than 0 / 1, n < 1, d < 1, ld < d, n * ld beyond 63 bits, B outside [1,
 * d3p_marginals_max_bins()]: D3P_E_INVALID_ARG; ws_bytes below n * d or a null ws_dev: D3P_E_WORKSPACE; a d whose pair tiles times
 * strips exceed 2^31 - 1 workgroups (which also keeps the pair tables within size_t): D3P_E_UNSUPPORTED; last, a pointer that is not device memory:
 * D3P_E_INVALID_ARG. */
int d3p_marginals(void* stream, const void* x_dev, int32_t dtype, int64_t ld, uint32_t n, uint32_t d, uint32_t B,
                  const uint32_t* nbins_dev,                  /* d */
                  const float* edges_dev,                     /* d x (B - 1) */
                  uint32_t* one_way_dev,                      /* d x K */
                  uint32_t* two_way_dev,                      /* d (d - 1) / 2 x K x K */
                  void* ws_dev, size_t ws_bytes);
/* host only, no device call: the largest B; the rows of a strip of the pair walk; the pairs a workgroup holds at once; the rows a
 * workgroup of the code kernel owns; the workspace in bytes (0: an argument out of range) */
uint32_t d3p_marginals_max_bins(void);
uint32_t d3p_marginals_strip_rows(void);
uint32_t d3p_marginals_pair_tile(void);
uint32_t d3p_marginals_code_rows(void);
size_t d3p_marginals_workspace(uint32_t n, uint32_t d, uint32_t B);

/* Label sums of the pooled pair distances (model-free; d3p_amd/permutation.py; d3p_label_sums.hip); added symbols, ABI 9
 * unchanged.  What a permutation test of the two-sample energy distance (Szekely & Rizzo; R's energy::eqdist.etest) needs of the pairs:
 * for R labellings g_r in {0, 1}^m of the m pooled rows the quadratic form of the distance matrix, in ONE O(m^2 (d + R)) walk that
 * computes every distance once -- never the m x m matrix, never a walk per labelling.
 * z_dev[i * ld + c] is pooled row i < m in column c < d (column stride 1), float32 (dtype 0) or int32 (dtype 1: converted to float32 when
 * staged, which is exact for |v| <= 2^24; the Python layer refuses larger magnitudes).  D_ij is d3p_pair_stats' distance, bit for bit
 * (both walk the tile of d3p_pair_tile.h):
 *   t_c = fl32(z_ic - z_jc),  q = the float32 fmaf chain over c ascending from 0,  D_ij = sqrtf(q) correctly rounded
 * so D_ii is exactly +0.0.  labels_dev is uint32, tile-major [ceil(m / 32)][R]: bit p of word (tile, r) says that row 32 tile + p carries
 * label 1 in labelling r.  Bits of rows >= m in the last tile's words are ignored, whatever they hold; the words are only ever read as
 * bits, so no content can move an address.  With g_i the live bit of row i:
 *   s11_dev[r] = sum_{i,j} g_i g_j (double)D_ij   in float64, in the fixed order d3p_label_sums.hip states, not rounded further
 *   s1t_dev[r] = sum_i g_i row_sum_dev[i]         over i ascending onto 0; a row that is not selected adds nothing
 *   n1_dev[r]  = the population count of the live bits
 * row_sum_dev is the caller's (d3p_pair_stats of z against itself); s1t propagates what it holds on the selected rows.  A NaN or +-inf
 * element anywhere in z makes every s11_dev[r] NaN (the flag taken while staging, never inf - inf); finite elements whose t_c or q
 * overflows float32 follow IEEE from there.
 * THE ORDER of s11[r]: rows in tiles of d3p_pair_label_sums_tile_rows() = 32, tile J in slot J mod 4; per (tile pair (I, J), r) and row ii
 * of tile I the row sum adds its 32 distances in ascending column onto 0 (a clear column bit adds +0.0); per (I, slot, r) the slot sum
 * adds the row sums of set row bits (a clear one adds +0.0) in ascending ii, then ascending J, onto 0; the four slot sums are added in
 * ascending order onto 0: the cell (I, r), a float64 of ws_dev; a second launch adds the cells in ascending I onto 0 and computes s1t and
 * n1.  One form.  A workgroup owns a tile I and a block of d3p_pair_label_sums_block_labellings() = 512 labellings, whose sums stay in
 * registers; R <= d3p_pair_label_sums_max_labellings() = 65536; d3p_pair_label_sums_workspace(m, d, R) = 8 R ceil(m / 32) bytes (0: an
 * argument out of range), every byte read is written in the same call.
 * Deterministic: no floating-point atomics, no host synchronisation; repeated calls give equal bits; s11[r] depends on z, m, d and
 * labelling r alone -- not on R, the other labellings, r's place in its group of 64 or its block, ld or the workspace's previous contents.
 * Checked before any launch, in this order: a null pointer (ws_dev may be null only where the workspace is 0, that is, where a later check
 * refuses the shape), a pointer not aligned to 4 bytes (row_sum_dev, s11_dev, s1t_dev, ws_dev: 8), a dtype other than 0 / 1, m < 1,
 * d < 1, ld < d, m * ld beyond 63 bits, R outside [1, d3p_pair_label_sums_max_labellings()]: D3P_E_INVALID_ARG; more than 2^31 - 1
 * workgroups (tiles x blocks; the message names them): D3P_E_UNSUPPORTED; ws_bytes below d3p_pair_label_sums_workspace: D3P_E_WORKSPACE,
 * with nothing touched; last, a pointer that is not device memory: D3P_E_INVALID_ARG. */
int d3p_pair_label_sums(void* stream, const void* z_dev, int32_t dtype, int64_t ld, uint32_t m, uint32_t d, uint32_t R,
                        const uint32_t* labels_dev,                 /* ceil(m / 32) x R */
                        const double* row_sum_dev,                  /* m */
                        double* s11_dev, double* s1t_dev, uint32_t* n1_dev,      /* R each */
                        void* ws_dev, size_t ws_bytes);
/* host only, no device call: the rows of a tile (32 = the bits of a label word); the labellings a workgroup owns; the largest R; the
 * workspace in bytes */
uint32_t d3p_pair_label_sums_tile_rows(void);
uint32_t d3p_pair_label_sums_block_labellings(void);
uint32_t d3p_pair_label_sums_max_labellings(void);
size_t d3p_pair_label_sums_workspace(uint32_t m, uint32_t d, uint32_t R);

#ifdef __cplusplus
}
#endif
#endif /* D3P_HIP_H */
