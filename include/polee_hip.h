/*
 * polee_hip.h -- C ABI of libpolee_hip.so, the MI355X (gfx950) approximate-likelihood
 * engine for Polee.  This is the drop-in boundary: the reference's Julia host code
 * reaches these symbols with `ccall` (see INTEGRATION.md and julia/PoleeHIP.jl); they
 * replace the PyCall + TensorFlow + hsb_ops.so path entirely.
 *
 * Conventions
 *   - Every function returns a polee_status (0 = ok).  A message for the last failure
 *     on a context is available from polee_last_error(ctx); failures that happen
 *     before a context exists are reported by polee_last_error(NULL).
 *   - Host pointers are borrowed for the duration of the call only (Julia callers
 *     must GC.@preserve them).  The library copies what it needs to the device.
 *     Pointers named d_* are DEVICE pointers.
 *   - Index arrays use the reference's on-disk conventions: node_parent_idxs, node_js,
 *     colptr, rowval are 1-based exactly as in the prep / likelihood-matrix HDF5 files;
 *     left/right/leaf_index are 0-based with -1 = none as make_inverse_ptt_params
 *     (src/ptt.jl:293-309) produces them for the TF ops.
 *   - Batched arrays are row-major [B][len].
 *   - One HIP stream per context; a handle must not be used from two host threads at
 *     once; different contexts (different GPUs) may be driven concurrently.  The
 *     library calls hipSetDevice itself on every entry (safe from any OS thread).
 *   - Nothing here falls back to the CPU: without a usable GPU polee_ctx_create fails.
 *
 * Citations are reference file:line, relative to the reference repository root.
 */
#ifndef POLEE_HIP_H
#define POLEE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int polee_status;
enum {
    POLEE_OK = 0,
    POLEE_ERR_BAD_ARG = 1,     /* size / NULL / malformed tree or matrix                  */
    POLEE_ERR_OOM = 2,         /* host or device allocation failed                        */
    POLEE_ERR_HIP = 3,         /* a HIP runtime call or kernel launch failed              */
    POLEE_ERR_NONFINITE = 4,   /* non-finite gradient / likelihood (mirrors the @assert   */
                               /* isfinite at likelihood-approximation.jl:559,564,        */
                               /* likelihood.jl:50, ptt.jl:156-157)                       */
    POLEE_ERR_UNSUPPORTED = 5, /* valid input outside what the kernels are built for      */
    POLEE_ERR_COMM = 6         /* collective / communicator failure                       */
};

typedef struct polee_ctx polee_ctx;       /* device + stream + error state               */
typedef struct polee_ptt polee_ptt;       /* one Polya tree transform (device resident)  */
typedef struct polee_loglik polee_loglik; /* one sample's X, device resident             */
typedef struct polee_vi polee_vi;         /* state of one likelihood-approximation fit   */
typedef struct polee_approx polee_approx; /* S fitted approximations (regression input)  */
typedef struct polee_regression polee_regression; /* regression model + surrogate posterior */

/* ---- context -------------------------------------------------------------------- */
polee_status polee_ctx_create(int device, polee_ctx **out);
void polee_ctx_destroy(polee_ctx *ctx);
const char *polee_last_error(const polee_ctx *ctx_or_null);
polee_status polee_ctx_synchronize(polee_ctx *ctx);
/* free / total device memory of the context's GPU (hipMemGetInfo), in bytes; either pointer may be NULL */
polee_status polee_ctx_mem_info(polee_ctx *ctx, int64_t *free_bytes, int64_t *total_bytes);
void *polee_ctx_stream(polee_ctx *ctx); /* the context's hipStream_t */
/* HIP-event stopwatch on the context's stream (bench.py times the hot path with it). */
polee_status polee_ctx_timer_start(polee_ctx *ctx);
polee_status polee_ctx_timer_stop(polee_ctx *ctx, double *elapsed_ms);
const char *polee_version(void);
/* The host-side builders (polee_loglik_create, polee_hclust*) keep the large scratch blocks they used for the next sample
 * (mapping and unmapping gigabytes per sample was a third of a sample's preparation): up to POLEE_HOST_CACHE_MB
 * megabytes; default = a quarter of the memory available to the process (MemAvailable, cut to the cgroup's
 * memory.max - memory.current), at most 8192.  A long-lived process therefore keeps up to that much resident after a
 * sample's preparation.  polee_host_cache_trim releases the blocks; polee_host_cache_configure sets a new cap in MB
 * (freeing what no longer fits; < 0: only query) and returns the cap in force; polee_host_cache_bytes = bytes cached now. */
void polee_host_cache_trim(void);
int64_t polee_host_cache_configure(int64_t cap_mb);
int64_t polee_host_cache_bytes(void);
/* DEVICE buffers likewise: what the library frees on the device (the builders' scratch, handles' arrays) is kept by size class
 * for the next allocation instead of going through hipFree / hipMalloc (a device-wide wait each, and multi-second stalls every few
 * samples) -- up to POLEE_DEVICE_CACHE_MB megabytes (default 65536; 0: off).  polee_host_cache_trim frees these too;
 * polee_device_cache_bytes = device bytes kept now. */
int64_t polee_device_cache_bytes(void);

/* ---- Polya tree transform ---------------------------------------------------------
 * Replaces PolyaTreeTransform (src/ptt.jl:6-27) and the three TF custom ops of
 * src/tensorflow_ext/hsb_ops.cpp.  The tree is given exactly as serialised in the
 * prep HDF5 (src/ptt.jl:89-116): N = 2n-1 nodes in DFS pre-order, right child first;
 * node_parent_idxs[i] = 1-based parent (0 for the root), node_js[i] = 1-based
 * transcript id of a leaf (0 for an internal node).  The k-th internal node in node
 * order owns ys[k]. */
polee_status polee_ptt_create(polee_ctx *ctx, const int32_t *node_parent_idxs,
                              const int32_t *node_js, int32_t N, polee_ptt **out);
/* Same tree given as the TF-op index arrays (src/ptt.jl:293-309; hsb_ops.cpp:17-22). */
polee_status polee_ptt_create_from_index(polee_ctx *ctx, const int32_t *left_index,
                                         const int32_t *right_index, const int32_t *leaf_index,
                                         int32_t N, polee_ptt **out);
void polee_ptt_destroy(polee_ptt *t);
int32_t polee_ptt_n(const polee_ptt *t); /* number of leaves (transcripts) */
/* make_inverse_ptt_params (src/ptt.jl:293-309), host only. */
polee_status polee_make_inverse_ptt_params(const int32_t *node_parent_idxs, const int32_t *node_js,
                                           int32_t N, int32_t *left_index, int32_t *right_index,
                                           int32_t *leaf_index);

/* transform! (src/ptt.jl:125-160): ys f64 [B][n-1] in [0,1] -> xs f32 [B][n] on the
 * simplex, leaves floored at 1e-16; ladj (optional, [B]) = sum over internal nodes of
 * log u.  A y of exactly 0 or 1 gives the subtree on its dead side u = 0: its leaves
 * come out at the floor, and ladj is -inf if that subtree has an internal node (a NaN
 * or +inf ladj is POLEE_ERR_NONFINITE).  The node values u of the last call stay on the device for
 * polee_ptt_transform_gradients, like t.us does in the reference. */
polee_status polee_ptt_transform(polee_ptt *t, const double *ys, int32_t B, float *xs,
                                 double *ladj_or_null);
/* transform_gradients! (src/ptt.jl:167-209) when with_ladj != 0, else
 * transform_gradients_no_ladj! (src/ptt.jl:217-251).  x_grad f64 [B][n] ->
 * y_grad f64 [B][n-1] (the reference stores f32; callers may round). */
polee_status polee_ptt_transform_gradients(polee_ptt *t, const double *ys, const double *x_grad,
                                           int32_t B, int with_ladj, double *y_grad);
/* inverse_transform! (src/ptt.jl:257-285): xs f32 [B][n] -> ys f64 [B][n-1],
 * ladj [B] = -sum log u. */
polee_status polee_ptt_inverse_transform(polee_ptt *t, const float *xs, int32_t B, double *ys,
                                         double *ladj_or_null);
/* TF op HSB (hsb_ops.cpp:17-120): logits f32 [B][n-1] -> x f32 [B][n]; no floor. */
polee_status polee_hsb(polee_ptt *t, const float *y_logit, int32_t B, float *x);
/* TF op InvHSB (hsb_ops.cpp:128-249): x f32 [B][n] -> y f64 [B][n-1], ladj f32 [B]. */
polee_status polee_inv_hsb(polee_ptt *t, const float *x, int32_t B, double *y, float *ladj);
/* TF op InvHSBGrad (hsb_ops.cpp:252-402): VJP of InvHSB. */
polee_status polee_inv_hsb_grad(polee_ptt *t, const double *y_grad, const float *ladj_grad,
                                const double *y, int32_t B, float *backprops);

/* ---- sparse fragment x transcript log-likelihood -----------------------------------
 * Replaces Model + log_likelihood + factored_log_likelihood (src/likelihood.jl:2-85)
 * and pAt_mul_B!/pAt_mulinv_B! (src/sparse.jl:6-40).  X is m x n in CSC form exactly
 * as stored in the likelihood-matrix HDF5 (src/rnaseq_sample.jl:505-519): colptr
 * [n+1] and rowval [nnz] 1-based; colptr may be uint32 (as the reference's UInt32
 * index type) or uint64 (colptr_bytes = 4 or 8).  ks (optional, [m]) are the integer
 * row multiplicities of the factored likelihood. */
polee_status polee_loglik_create(polee_ctx *ctx, int64_t m, int64_t n, const void *colptr,
                                 int colptr_bytes, const uint32_t *rowval, const float *nzval,
                                 const int64_t *ks_or_null, polee_loglik **out);
/* WHERE the device layout is built.  By default on the DEVICE (csrc/psell_device.hip): X is uploaded as given, transposed there
 * (a stable sort by fragment) and laid out by kernels that follow the host builder (csrc/psell_build.cpp) stage by stage -- byte
 * for byte the same layout (tests/test_gpu_device_build.py; 0.21 s at 20 M fragments x 200 k transcripts, against 0.73 s for the
 * host builder + upload).  The host builder takes over for a matrix without structure (a tenth of its non-zeros or more in
 * fragments that share no transcript set with their neighbours: stream C's question is sequential over all of them), for more
 * than 2^32 - 2 non-zeros, and when POLEE_DEVICE_BUILD=0 or one of its own experiment knobs (POLEE_PSELL_*) is set.
 * polee_loglik_built_on_device: 1 / 0 for a handle. */
int polee_loglik_built_on_device(const polee_loglik *ll);
/* Same sample given as Xt (n x m CSC == X in CSR), which the reference materialises
 * anyway (likelihood-approximation.jl:407): tcolptr [m+1] uint64 1-based row offsets,
 * trowval [nnz] 1-based transcript ids. */
polee_status polee_loglik_create_from_xt(polee_ctx *ctx, int64_t m, int64_t n,
                                         const uint64_t *tcolptr, const uint32_t *trowval,
                                         const float *tnzval, const int64_t *ks_or_null,
                                         polee_loglik **out);
void polee_loglik_destroy(polee_loglik *ll);

typedef struct {
    int64_t m, n, nnz;
    int64_t num_slices;      /* 64-row slices of the device layout                      */
    int64_t num_tiles;       /* workgroup-sized groups of slices                        */
    int64_t padded_nnz;      /* stored entries including padding                        */
    int64_t device_bytes;    /* bytes of X resident in HBM                              */
    int64_t stream_bytes;    /* bytes one likelihood pass streams from HBM (X only)     */
    int64_t num_empty_rows;  /* fragments with no compatible transcript (skipped)       */
    int32_t max_row_nnz;
    int32_t max_tile_cols;   /* largest per-tile column dictionary                      */
    /* the row streams of the device layout (see polee_amd/csrc/loglik_internal.hpp):                     */
    /* [0] dense uniform slices, sets of <= 16 transcripts; [1] masked uniform slices,   */
    /* unions of <= 16 (fragments whose sets differ); [2] dense uniform, 17..32; [3] masked uniform,    */
    /* unions of 17..32; [4] mixed slices of unrelated fragments of <= 15 transcripts -- [0..4] are one */
    /* persistent launch; [5] mixed slices of longer fragments (more than 32 transcripts, as a rule): a */
    /* second launch; [6] rows kept in CSR (fragments without any structure, whose sliced forms would   */
    /* cost more than CSR: a random sparse matrix): a launch of their own, no tiles; [7] fragments       */
    /* compatible with ONE transcript: collapsed at build time into a count per transcript (each adds    */
    /* log X_ij + log x_j to lp and 1 / x_j to the gradient): stream_bytes_hbm[7] = 4 n, no tiles        */
    int64_t stream_rows[8];  /* fragments                                               */
    int64_t stream_nnz[8];   /* non-zeros of X                                          */
    int64_t stream_tiles[8]; /* tiles (workgroup-sized units of work)                   */
    int64_t stream_bytes_hbm[8]; /* bytes of the slice stream a pass reads                */
    int64_t dict_entries;    /* entries of all tile dictionaries: x is gathered into, and the gradient flushed */
                             /* from, one window of dict_entries x K floats per pass                           */
} polee_loglik_info;
polee_status polee_loglik_get_info(const polee_loglik *ll, polee_loglik_info *info);
/* Deterministic mode ("fixed reduction order ... bitwise stable"): the gradient (and lp) of a pass is
 * summed in a fixed order -- per wave, per tile, then per transcript in tile order -- instead of with float atomics, so
 * that two evaluations on the same inputs agree bit for bit (and with them a whole fit with the same noise), whichever
 * workgroup takes which tile.  About 11 % slower (three workgroups per CU instead of four, a second small kernel).  Rows kept
 * in CSR (polee_loglik_info.stream_rows[6] > 0: fragments without any set structure, none in any input met so far) are
 * still added with float atomics: the guarantee holds when that stream is empty.  Default off. */
polee_status polee_loglik_set_deterministic(polee_loglik *ll, int on);

/* log_likelihood (src/likelihood.jl:36-56) for K expression vectors at once:
 * xs f32 [K][n] -> x_grad f64 [K][n] = sum_i X_ij / s_i  (x ks_i if factored);
 * lp [K] = sum_i log s_i (x ks_i) unless lp_or_null == NULL ("gradonly"). 1 <= K <= 8.
 * A polee_loglik supports ONE evaluation in flight at a time (polee_loglik_eval, or a polee_vi / polee_regression step that uses
 * the handle): the dynamic tile schedule keeps a per-handle counter on the device and its base on the host, and two threads or
 * streams evaluating the same handle at once would hand out wrong tiles.  Different handles are independent. */
polee_status polee_loglik_eval(polee_loglik *ll, const float *xs, int32_t K, double *x_grad,
                               double *lp_or_null);
/* effective_length_jacobian_adjustment! (src/likelihood.jl:93-110), batched:
 * x_grad[k][j] -= n / (efflens[j] * sum_i xs[k][i]/efflens[i]); xls optional out. */
polee_status polee_efflen_jacobian_adjustment(polee_ctx *ctx, const float *efflens, const float *xs,
                                              int32_t K, int64_t n, double *x_grad,
                                              float *xls_or_null);

/* gene_noninformative_prior! (src/likelihood.jl:114-159), batched over K draws: gradient of the
 * non-informative prior over gene-level expression.  gene_of int32[n] = gene index of each transcript
 * (0-based, -1 = no gene known): the reference's Dict{gene id -> transcript indexes} as an array.
 * xls f32 [K][n] is the output of polee_efflen_jacobian_adjustment; x_grad f64 [K][n] is updated. */
polee_status polee_gene_noninformative_prior(polee_ctx *ctx, const float *efflens, const float *xls,
                                             const float *xs, int32_t K, int64_t n, const int32_t *gene_of,
                                             double *x_grad);

/* ---- element-wise reparameterisations (standalone forms) --------------------------------
 * The Julia functions of src/logitnormal.jl:8-55, src/sinh_arcsinh.jl:10-38 and
 * src/kumaraswamy.jl:27-78 (inside the VI loop the first two are fused into the tree kernels).
 * Gradient entry points ACCUMULATE into *_grad like the reference's `+=`.  ladj pointers may be
 * NULL (= Val(false)). */
polee_status polee_logit_normal_transform(polee_ctx *ctx, const float *mu, const float *sigma,
                                          const float *zs, int64_t len, double *ys, double *ladj_or_null);
polee_status polee_logit_normal_transform_gradients(polee_ctx *ctx, const float *zs, const double *ys,
                                                    const float *sigma, const float *y_grad, int64_t len,
                                                    float *z_grad_or_null, float *mu_grad, float *sigma_grad);
polee_status polee_sinh_asinh_transform(polee_ctx *ctx, const float *alpha, const float *zs0, int64_t len,
                                        float *zs, double *ladj_or_null);
polee_status polee_sinh_asinh_transform_gradients(polee_ctx *ctx, const float *zs0, const float *alpha,
                                                  const float *z_grad, int64_t len, float *alpha_grad);
polee_status polee_kumaraswamy_transform(polee_ctx *ctx, const float *as, const float *bs, const float *zs,
                                         int64_t len, double *ys, double *ladj_or_null);
polee_status polee_kumaraswamy_transform_gradients(polee_ctx *ctx, const float *zs, const float *as,
                                                   const float *bs, const float *y_grad, int64_t len,
                                                   float *a_grad, float *b_grad);

/* ---- likelihood approximation (the VI loop) ----------------------------------------
 * Replaces approximate_likelihood(::LogitSkewNormalPTTApprox, sample)
 * (src/likelihood-approximation.jl:395-575), its factored variant (:248-392), ADAM
 * (:107-146) and the element-wise reparameterisations (src/logitnormal.jl:8-55,
 * src/sinh_arcsinh.jl:10-38).  Defaults are the reference's constants
 * (src/constants.jl:48-65, likelihood-approximation.jl:421-423). */
typedef struct {
    int32_t num_steps;           /* LIKAP_NUM_STEPS = 500                                  */
    int32_t num_mc_samples;      /* LIKAP_NUM_MC_SAMPLES = 6 (1..8)                        */
    int32_t use_efflen_jacobian; /* default 1 (--no-efflen-jacobian clears it)             */
    int32_t gradonly;            /* default 1: no ELBO / log-likelihood values             */
    uint64_t seed;               /* device Philox seed (reference default 123456789)       */
    const float *z0;             /* optional HOST noise [num_steps][num_mc][n-1]; when set */
                                 /* it replaces the device RNG (deterministic parity runs) */
    double y_eps;                /* LIKAP_Y_EPS = 1e-10 clamp of ys and xs; must lie in (0, 0.5) */
    double adam_initial_learning_rate; /* 1.0  */
    double adam_learning_rate_decay;   /* 2e-2 */
    double adam_min_learning_rate;     /* 1e-3 */
    double adam_eps;                   /* 1e-8 */
    double adam_rv;                    /* 0.9  */
    double adam_rm;                    /* 0.7  */
    double max_mu_step, max_omega_step, max_alpha_step; /* 0.2, 0.2, 0.02 */
    int32_t profile;             /* 1: bracket every sparse-kernel launch with HIP events; N > 1: every N-th launch (four
                                    event records per pass cost ~20 us of stream gaps per iteration at C2) */
    int32_t deterministic;       /* 1: this fit's likelihood passes run in deterministic mode (the handle's own  */
                                 /* polee_loglik_set_deterministic setting is untouched); -1: float atomics;      */
                                 /* 0 (default): deterministic exactly when the sample is shared by more than    */
                                 /* one rank (polee_vi_set_comm), so that repeated N-rank fits are bitwise equal  */
    const int32_t *gene_of;      /* optional HOST int32[n]: gene index of every transcript (0-based, -1 = none   */
                                 /* known) = gene_noninformative = true (likelihood-approximation.jl:475-491,     */
                                 /* 535-538: gene_noninformative_prior! after the effective-length adjustment,   */
                                 /* which it needs: use_efflen_jacobian must be on).  NULL: off (the CLI default) */
} polee_vi_opts;
void polee_vi_default_opts(polee_vi_opts *opts);

typedef struct {
    int32_t steps_done;
    int32_t nonfinite_step;        /* first step with a non-finite gradient, 0 if none    */
    double loglik_kernel_ms_avg;   /* profile=1: mean duration of the dominant sparse     */
                                   /* kernel (the persistent launch over the uniform streams) */
    int64_t loglik_kernel_launches;
    double last_elbo;              /* !gradonly: reference-style elbo of the last step    */
    double last_lp_mean;           /* !gradonly: mean log-likelihood over the K draws     */
    double loglik_pass_ms_avg;     /* profile=1: mean duration of one whole likelihood    */
                                   /* pass: the x-window gather, the persistent launch     */
                                   /* and, if the sample has mixed tiles, their launch     */
} polee_vi_stats;

/* Builds the state and the initial values mu = logit(inverse_transform(1/n)),
 * omega = log 0.1, alpha = 0 (likelihood-approximation.jl:451-456). */
polee_status polee_vi_create(polee_loglik *ll, polee_ptt *t, const float *efflens,
                             const polee_vi_opts *opts, polee_vi **out);
void polee_vi_destroy(polee_vi *vi);
/* Enqueues nsteps VI iterations (K draws + one ADAM update each) on the context's
 * stream without host synchronisation. */
polee_status polee_vi_run(polee_vi *vi, int32_t nsteps);
/* Waits for the stream; returns POLEE_ERR_NONFINITE if any step met a non-finite
 * gradient (likelihood-approximation.jl:559). */
polee_status polee_vi_sync(polee_vi *vi);
polee_status polee_vi_get_params(polee_vi *vi, float *mu, float *omega, float *alpha);
polee_status polee_vi_set_params(polee_vi *vi, const float *mu, const float *omega,
                                 const float *alpha);
polee_status polee_vi_get_stats(polee_vi *vi, polee_vi_stats *stats);
/* Per-step values recorded when gradonly == 0: elbo [steps_done] as the reference
 * computes it (last draw's lp + ladj, divided by K: likelihood-approximation.jl:537,
 * 561) and the mean log-likelihood over draws.  Either pointer may be NULL. */
polee_status polee_vi_get_trace(polee_vi *vi, double *elbo, double *lp_mean);
/* The noise the device RNG uses at (step, draw): z0 f32 [K][n-1] for 1-based step. */
polee_status polee_vi_export_noise(polee_vi *vi, int32_t step, float *z0);
/* Test hook: evaluates the K draws of the NEXT step at the current parameters and
 * returns the step's averaged gradients (what ADAM would consume), without updating
 * anything.  Any output may be NULL.  xs [K][n], x_grad [K][n] (after the effective
 * length adjustment), y_grad [K][n-1], *_grad [n-1], lp [K], ladj [K]. */
polee_status polee_vi_eval_gradients(polee_vi *vi, float *xs, double *x_grad, double *y_grad,
                                     float *mu_grad, float *omega_grad, float *alpha_grad,
                                     double *lp, double *ladj);
/* approximate_likelihood in one call: create + run(num_steps) + sync + get_params. */
polee_status polee_vi_fit(polee_loglik *ll, polee_ptt *t, const float *efflens,
                          const polee_vi_opts *opts, float *mu, float *omega, float *alpha,
                          polee_vi_stats *stats_or_null);

/* approximate_likelihood(::OptimizePTTApprox, sample) (src/likelihood-approximation.jl:149-242): point
 * optimisation of the expression vector by ADAM ascent on z (ys = logistic(z)), used by the reference to
 * assign reads while fitting bias models (src/rnaseq_sample.jl:343).  The reference builds a :sequential
 * tree itself; here the tree is the caller's.  xs f32 [n] (clamped to [1e-10, 1]); zs optional f32 [n-1]. */
polee_status polee_optimize_ptt(polee_loglik *ll, polee_ptt *t, const float *efflens, int32_t num_steps,
                                float *xs, float *zs_or_null);

/* ---- tree construction (host side) --------------------------------------------------------
 * hclust + order_nodes (src/hclust.jl:193-319, 361-389), the heuristic behind
 * PolyaTreeTransform(X, :cluster) (src/ptt.jl:35-52): greedy joining of the transcripts / subtrees that share
 * the most reads (Jaccard similarity of read sets among 25 neighbours in median-read order), remaining
 * components smallest first, nodes in DFS pre-order, right child first.  X in CSC, 1-based, as in the
 * likelihood-matrix HDF5.  Outputs int32 [2n-1] each: exactly the arrays polee_ptt_create takes and the prep
 * HDF5 stores.  Runs on the CPU (as the reference's does); no context needed. */
polee_status polee_hclust(int64_t m, int64_t n, const void *colptr, int colptr_bytes, const uint32_t *rowval,
                          int32_t *node_parent_idxs, int32_t *node_js);
/* The same rule -- join the subtrees that share the most reads first -- in parallel rounds: every round merges each edge
 * that is the best edge (similarity, then a hash of the endpoints: a total order) of both its endpoints, on all host
 * threads; new nodes are numbered by their edges' priorities, so the tree does not depend on the thread count.  Not the
 * reference's tree node for node (its order depends on heap positions among equal similarities, which no parallel
 * schedule reproduces, and a locally best edge is merged before a better one can appear at an endpoint): a documented
 * variant for sample preparation at scale (polee_amd/csrc/hclust.cpp; the exact mode above stays the default).  Same
 * arguments, same output arrays. */
polee_status polee_hclust_parallel(int64_t m, int64_t n, const void *colptr, int colptr_bytes, const uint32_t *rowval,
                                   int32_t *node_parent_idxs, int32_t *node_js);
/* The same tree -- node for node the arrays polee_hclust_parallel gives -- built on the DEVICE (csrc/hclust_device.hip): per round the
 * best live edge of every node by atomic maxima over the priorities, the mutually-best edges sorted by priority, their read
 * sets united and the similarities to the neighbours of both halves counted by binary searches spread over the whole GPU. */
polee_status polee_hclust_parallel_device(polee_ctx *ctx, int64_t m, int64_t n, const void *colptr, int colptr_bytes,
                                          const uint32_t *rowval, int32_t *node_parent_idxs, int32_t *node_js);

/* ---- tree from transcript sequences: polee fit-tree (src/main.jl:638-660) ------------------
 * The definition is this project's own: upstream's k-mer hash is Julia's and its merge order among equal
 * similarities depends on heap positions.  Upstream's constants are kept (src/constants.jl:88-89). */
#define POLEE_KMER_K 32
#define POLEE_KMER_H 200
/* most transcripts a tree is built for (n * 200 sketch entries are indexed with 32 bits) */
#define POLEE_KMER_MAX_N 10000000LL
/* most co-occurring pairs of transcripts the candidate-edge step emits (8 bytes each, sorted out of place): a k-mer that r
 * transcripts share gives r (r - 1) / 2 pairs, so repeat-derived k-mers shared by thousands of transcripts grow quadratically.
 * Counted before anything is allocated; above the limit the builders return POLEE_ERR_BAD_ARG. */
#define POLEE_KMER_MAX_PAIRS (1LL << 30)
/* windows (k-mer start positions) one workgroup of the sketch kernel covers: a longer transcript is split over several */
#define POLEE_KMER_SKETCH_CHUNK 8192
/* One-permutation MinHash sketches of the transcripts' canonical 32-mers (replaces KmerSketch(seq), src/kmersketch.jl:7-40,
 * with the hash and the bin rule of DESIGN.md 3.12).  bases: the transcripts' ASCII bytes concatenated (A C G T in either
 * case; any other byte breaks the windows that touch it), transcript t = bases[offsets[t] .. offsets[t+1]), offsets[0] = 0.
 * sketches: uint64 [n][200], 0 = empty bin.  Bitwise reproducible (a minimum does not depend on order). */
polee_status polee_kmer_sketch(polee_ctx *ctx, int64_t n, const int64_t *offsets, const uint8_t *bases, uint64_t *sketches);
/* the same sketches on the host threads, no context (what `fit_tree --host` uses) */
polee_status polee_kmer_sketch_host(int64_t n, const int64_t *offsets, const uint8_t *bases, uint64_t *sketches);
/* The tree of n sketches (replaces build_polya_tree_transformation / cluster, src/kmercluster.jl:96-262, and order_nodes,
 * :69-93; similarity and union as src/kmersketch.jl:43-67): greedy joining by approximate Jaccard, ties by smaller node numbers,
 * the rest joined Huffman-fashion, nodes in DFS pre-order, right child first.  Outputs int32 [2n-1] each, the arrays
 * polee_ptt_create takes.  Host only, no context; POLEE_ERR_BAD_ARG for a sketch value outside its bin. */
polee_status polee_kmer_tree_host(int64_t n, const uint64_t *sketches, int32_t *node_parent_idxs, int32_t *node_js);
/* the same tree, node for node: the candidate edges (every pair of sketches that shares a bin value, with the number of shared
 * and of jointly empty bins) come from the device -- one sort of the sketch entries, one of the pair keys -- the merge loop
 * runs on the host (replaces the index / queue set-up, src/kmercluster.jl:107-190) */
polee_status polee_kmer_tree(polee_ctx *ctx, int64_t n, const uint64_t *sketches, int32_t *node_parent_idxs, int32_t *node_js);
/* polee_kmer_sketch + polee_kmer_tree with the sketches left on the device in between (polee fit-tree, src/main.jl:638-649) */
polee_status polee_fit_tree(polee_ctx *ctx, int64_t n, const int64_t *offsets, const uint8_t *bases, int32_t *node_parent_idxs,
                            int32_t *node_js);
/* The same inputs and outputs with the Jaccard merges made in ROUNDS ("merge in rounds"): every round merges each
 * edge that is the best edge of both its endpoints -- priority: bits of J, a hash of the two node numbers, the smaller numbers --
 * and numbers the new nodes in the order of the priorities.  Another tree than the greedy one (a heuristic either way), the same
 * tree from all three entries, whatever the thread count or the launch geometry.  stats: NULL, or int64 [4] = {rounds, merges,
 * nodes left for the Huffman phase, pairs re-evaluated}.  _host: host threads only, no context.  polee_kmer_tree_rounds: index
 * and rounds on the device, nothing of the index is copied to the host.  polee_fit_tree_rounds: sketches on the device as well. */
polee_status polee_kmer_tree_rounds_host(int64_t n, const uint64_t *sketches, int32_t *node_parent_idxs, int32_t *node_js, int64_t *stats);
polee_status polee_kmer_tree_rounds(polee_ctx *ctx, int64_t n, const uint64_t *sketches, int32_t *node_parent_idxs, int32_t *node_js,
                                    int64_t *stats);
polee_status polee_fit_tree_rounds(polee_ctx *ctx, int64_t n, const int64_t *offsets, const uint8_t *bases, int32_t *node_parent_idxs,
                                   int32_t *node_js, int64_t *stats);

/* ---- one sample over several GPUs -----------------------------------
 * X's rows (fragments) are sharded over the ranks in contiguous blocks; every rank creates its
 * polee_loglik from its block and runs the same polee_vi (same seed => identical state); per
 * likelihood pass the partial gradients (K*n f32) and log-likelihoods are summed with one
 * all-reduce over RCCL (bound at run time).  One rank calls polee_comm_unique_id and the caller
 * distributes the 128 bytes (MPI, torch.distributed, a file ...). */
typedef struct polee_comm polee_comm;
#define POLEE_COMM_ID_BYTES 128
polee_status polee_comm_unique_id(uint8_t id[POLEE_COMM_ID_BYTES]);
polee_status polee_comm_create(polee_ctx *ctx, int32_t nranks, int32_t rank,
                               const uint8_t id[POLEE_COMM_ID_BYTES], polee_comm **out);
/* The same communicator interface over a HOST all-reduce supplied by the caller (MPI_Allreduce, a torch.distributed
 * gloo group, ...): the library stages the buffer through host memory (stream-synchronising; for clusters without
 * RCCL between the ranks, and for tests that run two ranks on one GPU).  `allreduce(user, buf, count, is_f64)` must sum
 * `buf` (count f32 / f64 values) over all ranks in place and return 0. */
typedef int (*polee_host_allreduce_fn)(void *user, void *buf, int64_t count, int is_f64);
polee_status polee_comm_create_host(polee_ctx *ctx, int32_t nranks, int32_t rank, polee_host_allreduce_fn allreduce,
                                    void *user, polee_comm **out);
void polee_comm_destroy(polee_comm *comm);
int32_t polee_comm_rank(const polee_comm *comm);
int32_t polee_comm_size(const polee_comm *comm);
/* what the transport itself reports: *transport = 1 RCCL / 2 host-staged; *count, *user_rank = ncclCommCount,
 * ncclCommUserRank of the RCCL communicator (the creation arguments for a host communicator); any pointer may be NULL */
polee_status polee_comm_info(const polee_comm *comm, int32_t *transport, int32_t *count, int32_t *user_rank);
/* sum over ranks of a host buffer (convenience; the VI loop reduces device buffers in place) */
polee_status polee_allreduce_sum_f32(polee_comm *comm, float *buf, int64_t count);
/* make `vi` a row-sharded fit: its likelihood handle holds this rank's block of rows */
polee_status polee_vi_set_comm(polee_vi *vi, polee_comm *comm_or_null);

/* ---- sampler ------------------------------------------------------------------------
 * rand!(::ApproxLikelihoodSampler) (src/approx-sampler.jl:37-44): draws x f32
 * [ndraws][n] from a fitted approximation.  z0 (optional host [ndraws][n-1]) replaces
 * the device RNG.  No clamp, leaves floored at 1e-16 by transform!. */
polee_status polee_sampler_draw(polee_ptt *t, const float *mu, const float *sigma,
                                const float *alpha, const float *z0_or_null, int32_t ndraws,
                                uint64_t seed, float *xs);

/* Initial values of the model entry, load_samples_hdf5 (src/estimate.jl:436-455): the mean of ndraws (30 there) draws
 * z0 -> sinh-asinh -> logistic, y clamped to [LIKAP_Y_EPS, 1 - LIKAP_Y_EPS] -> transform!, each draw divided by the
 * effective lengths and renormalised; x0 f32 [n].  z0 as in polee_sampler_draw. */
polee_status polee_sampler_initial_values(polee_ptt *t, const float *mu, const float *sigma, const float *alpha,
                                          const float *efflens, const float *z0_or_null, int32_t ndraws,
                                          uint64_t seed, float *x0);

/* posterior_mean (src/approx-sampler.jl:86-117): mean over ndraws draws, each clamped to [1e-15, 0.9999999]
 * (f32 accumulation in draw order, as the reference); pm f32 [n].  z0 as in polee_sampler_draw. */
polee_status polee_sampler_posterior_mean(polee_ptt *t, const float *mu, const float *sigma, const float *alpha,
                                          const float *z0_or_null, int32_t ndraws, uint64_t seed, float *pm);
/* Statistics.quantile(loaded_samples, transforms, qs, N) for one sample (src/approx-sampler.jl:50-83): element-wise
 * quantiles (Julia's default definition, linear interpolation between order statistics) of ndraws draws;
 * qs f64 [nq] (nq <= 8), quantiles f32 [nq][n]. */
polee_status polee_sampler_quantiles(polee_ptt *t, const float *mu, const float *sigma, const float *alpha,
                                     const float *z0_or_null, int32_t ndraws, uint64_t seed, const double *qs,
                                     int32_t nq, float *quantiles);

/* ---- density of fitted approximations (regression consumer) --------------------------
 * Replaces RNASeqApproxLikelihoodDist._log_prob (src/polee_approx_likelihood.py:367-450)
 * and, with it, the InvHSB/InvHSBGrad ops inside TF's autodiff.  S samples, each with
 * its own tree (or one shared tree when shared_tree != 0: index arrays are [1][N]).
 * Arrays follow create_tensorflow_variables! (src/estimate.jl:502-556): efflens
 * [S][n], la_mu/la_sigma/la_alpha [S][n-1], left/right/leaf_index int32 [S][N]. */
polee_status polee_approx_create(polee_ctx *ctx, int32_t S, int32_t n, const float *efflens,
                                 const float *la_mu, const float *la_sigma, const float *la_alpha,
                                 const int32_t *left_index, const int32_t *right_index,
                                 const int32_t *leaf_index, int shared_tree, polee_approx **out);
void polee_approx_destroy(polee_approx *ap);
/* x f32 [S][n] unnormalised log-expression -> lp f32 [S]; x_grad (optional, [S][n]) =
 * d lp[s] / d x[s][:]. */
polee_status polee_approx_logprob(polee_approx *ap, const float *x, float *lp,
                                  float *x_grad_or_null);
/* Same on device buffers, enqueued on the context's stream (no host sync). */
polee_status polee_approx_logprob_device(polee_approx *ap, const float *d_x, float *d_lp,
                                         float *d_x_grad_or_null);
/* RNASeqGeneApproxLikelihoodDist (src/polee_gene_expression.py:14-90): the same density reached through
 * gene-level expression.  x[s][i] = x_gene[s][g(i)] + x_isoform[s][i] - logsumexp_{i' in g(i)} x_isoform[s][i']
 * (the reference's exp / blockwise sparse matmul / log), then _log_prob of the transcript approximation.
 * gene_of int32 [n]: 0-based gene of every transcript (each transcript in exactly one gene, every gene
 * non-empty).  lp f32 [S]; gradients (optional) d lp[s] / d x_gene [S][G] and / d x_isoform [S][n]. */
polee_status polee_approx_gene_logprob(polee_approx *ap, const float *x_gene, const float *x_isoform,
                                       const int32_t *gene_of, int32_t num_genes, float *lp,
                                       float *gene_grad_or_null, float *isoform_grad_or_null);
/* rnaseq_approx_likelihood_sampler (src/polee_approx_likelihood.py:35-59): one draw per
 * sample, divided by efflens, renormalised and clipped to [1e-16, 0.99999999].
 * z0 optional host [S][n-1]. */
polee_status polee_approx_sample(polee_approx *ap, const float *z0_or_null, uint64_t seed,
                                 float *x);

/* approximate_feature_likelihood (src/polee_gene_expression.py:191-222): a normal approximation of the log
 * expression of FEATURES (sets of transcripts, typically genes), by moments of sampler draws: loc = mean over
 * num_mean_draws draws of log sum_{t in feature} x_t (x from polee_approx_sample's sampler), scale = sqrt of the mean
 * squared deviation from loc over a further num_var_draws draws.  The feature / transcript incidence comes as
 * num_pairs (feature, transcript) pairs, 1-based (transcript_expression_to_feature_expression, :163-173).
 * z0 (optional, tests) = noise of all draws, host [(num_mean_draws + num_var_draws)][S][n-1].
 * loc, scale: f32 [S][F].  (The reference runs 1000 + 1000 draws.) */
polee_status polee_approx_feature_moments(polee_approx *ap, const int32_t *feature_idxs, const int32_t *transcript_idxs,
                                          int64_t num_pairs, int32_t F, int32_t num_mean_draws, int32_t num_var_draws,
                                          uint64_t seed, const float *z0_or_null, float *loc, float *scale);

/* approximate_splicing_likelihood (src/polee_splicing.py:47-113): the same moments for splicing log-ratios,
 * log sum_{t in feature} x_t - log sum_{t in antifeature} x_t.  feature_indices / antifeature_indices: int32 [P][2] /
 * [Q][2] rows (feature, transcript), 0-based, as the reference's NumPy arrays. */
polee_status polee_approx_splicing_moments(polee_approx *ap, const int32_t *feature_indices, int64_t num_feature_pairs,
                                           const int32_t *antifeature_indices, int64_t num_antifeature_pairs, int32_t F,
                                           int32_t num_mean_draws, int32_t num_var_draws, uint64_t seed,
                                           const float *z0_or_null, float *loc, float *scale);

/* ---- regression model ---------------------------------------------
 * Replaces RNASeqLinearRegression.__init__ / model_fn / variational_model_fn / fit
 * (models/polee_regression.py:18-340): the horseshoe+ linear model of log expression with kernel-regression
 * mean-variance and distortion terms, its mean-field surrogate posterior, and
 * tfp.vi.fit_surrogate_posterior(sample_size = 1, Adam(2e-3)) as hand-derived gradients of
 * loss = log q(z) - log p(z) at one reparameterised draw z per step.
 *   ap            fitted approximations of the S samples (the likelihood term, polee_approx_likelihood.py:367-450);
 *                 NULL or use_point_estimates != 0: no likelihood term, x fixed at x_init (qx_loc not trained)
 *   design        f32 [S][F] factor matrix;  x_init f32 [S][n] log expression;  sample_scales f32 [S]
 *   x_init_mean   f32 [n] column means of x_init over ALL samples, or NULL to take them from x_init (needed when
 *                 this handle holds one rank's shard of the samples, see polee_regression_set_comm)
 *   hinges        f32 [degree] kernel-regression knots, or NULL for choose_knots(min, max of the column means of
 *                 x_init) as RNASeqTranscriptLinearRegression does (models/polee_regression.py:436-440)
 *   x_bias_loc0 / x_bias_scale0   prior of x_bias (log(1/n) and 12 in the reference's subclasses)
 * Flat parameter (and gradient) vector, each array row-major, in this order (the reference's variable names
 * without "_var"):  qw_global_scale_variance_loc, .._softplus_scale, qw_global_scale_noncentered_loc,
 * .._softplus_scale (4 scalars); qw_distortion_c_loc [F][degree]; qx_scale_concentration_c_loc [degree];
 * qx_scale_scale_c_loc [degree]; then [F][n] each: qw_local1_scale_variance_{loc,softplus_scale},
 * qw_local1_scale_noncentered_{..}, qw_local2_scale_variance_{..}, qw_local2_scale_noncentered_{..}, qw_loc,
 * qw_softplus_scale; then [n] each: qx_bias_loc, qx_bias_softplus_scale, qx_scale_loc, qx_scale_softplus_scale;
 * then [S][n] each: qx_loc, qx_softplus_scale.
 * Noise vector (standard normals of the draw): w_global_scale_variance, w_global_scale_noncentered (2 scalars);
 * [F][n] each: w_local1_scale_variance, w_local1_scale_noncentered, w_local2_.., w_local2_.., w; x_bias [n];
 * x_scale [n]; x [S][n]. */
polee_status polee_regression_create(polee_ctx *ctx, polee_approx *ap_or_null, int32_t S, int32_t F, int32_t n,
                                     const float *design, const float *x_init, const float *x_init_mean_or_null,
                                     const float *sample_scales, const float *hinges_or_null, int32_t degree,
                                     float bandwidth, float x_bias_loc0, float x_bias_scale0, int use_distortion,
                                     float scale_penalty, int use_point_estimates, polee_regression **out);
void polee_regression_destroy(polee_regression *reg);
int64_t polee_regression_num_params(const polee_regression *reg);
int64_t polee_regression_num_noise(const polee_regression *reg);
polee_status polee_regression_get_params(polee_regression *reg, float *params);
polee_status polee_regression_set_params(polee_regression *reg, const float *params);
/* RNASeqNormalTranscriptLinearRegression (models/polee_regression.py:490-531): replace the likelihood term by
 * point estimates with a scale, loc[s][j] ~ Normal(log softmax(x[s])[j], scale[s][j]); loc, scale f32 [S][n]. */
polee_status polee_regression_set_normal_likelihood(polee_regression *reg, const float *loc, const float *scale);
/* RNASeqGeneLinearRegression (models/polee_regression.py:533-600): the model's n features are GENES and the
 * likelihood is RNASeqGeneApproxLikelihoodDist (polee_approx_gene_logprob) of (x_gene, x_isoform), with
 * x_isoform_mean ~ Normal(0, 2) [nt], x_isoform ~ Normal(x_isoform_mean, 1) [S][nt] and Normal surrogates for both.
 * Create the model with ap = NULL over the genes, then attach: ap over the nt transcripts, gene_of int32 [nt]
 * (0-based gene of every transcript), x_isoform_init f32 [S][nt].  Adds an isoform block of parameters (own Adam
 * state): qx_isoform_mean_loc [nt], qx_isoform_mean_softplus_scale [nt], qx_isoform_loc [S][nt],
 * qx_isoform_softplus_scale [S][nt]; and appends noise (mean [nt], isoform [S][nt]) to the noise vector. */
polee_status polee_regression_set_gene_likelihood(polee_regression *reg, polee_approx *ap, const int32_t *gene_of,
                                                  const float *x_isoform_init);
/* RNASeqGeneIsoformLinearRegression (models/polee_regression.py:656-877): as above, but the isoform block is a
 * regression of its own over the nt transcripts: x_isoform ~ Normal(x_isoform_bias + F_isoform w_isoform,
 * x_isoform_scale) with horseshoe+ coefficients w_isoform [Fi][nt] (:698-720), x_isoform_bias ~ Normal(0, 2) (:722-724),
 * x_isoform_scale ~ InverseGamma(0.001, 0.001) (:728-729) and the surrogates of :736-833.  design_isoform f32 [S][Fi].
 * The isoform block then holds, in this order (the model's own order with the isoform design and no hinges):
 * global scale variance loc / softplus_scale, global scale noncentered loc / softplus_scale; [Fi][nt] arrays local1
 * variance loc / s, local1 noncentered loc / s, local2 variance loc / s, local2 noncentered loc / s, w loc / s;
 * [nt] arrays bias loc / s, scale loc / s; [S][nt] arrays x_isoform loc / s.  Noise appended to the noise vector: 2
 * globals, five [Fi][nt] arrays (the four scales, w), bias [nt], scale [nt], x_isoform [S][nt]. */
polee_status polee_regression_set_gene_isoform_likelihood(polee_regression *reg, polee_approx *ap,
                                                          const int32_t *gene_of, const float *x_isoform_init,
                                                          const float *design_isoform, int32_t num_isoform_factors);
/* RNASeqJointLinearRegression (models/polee_regression.py:879-1283; driven by models/joint-regression.jl): gene-level
 * regression + a regression over SPLICE FEATURES whose predictor reaches the transcripts through the 0/1 feature matrix.
 * Create the model over the gene features with ap = NULL, use_distortion = 0, scale_penalty = 5e-4 (:1052-1054), then
 * attach: ap over the nt transcripts, gene_of int32 [nt], x_isoform_init f32 [S][nt], the number of splice features P and
 * the matrix's non-zeros as (transcript, feature) pairs, 0-based.  The gene block becomes the joint model's: a horseshoe
 * prior (ONE local scale level: the local2 arrays of the flat vector stay, unused), kernel-regression weights that follow
 * the SAMPLED bias (:1034-1035), HalfCauchy(0, 10) on the mean-variance coefficients (:1037-1041),
 * qw_softplus_scale = -2, Adam(1e-3) (:1215).  The isoform block then holds: the splice block in the model's own order
 * with P columns and no hinges -- global scale variance loc / s, noncentered loc / s; [F][P] arrays local variance loc / s,
 * local noncentered loc / s, (local2: four unused arrays), w_splice loc / s; [P] arrays bias loc / s, (x_scale: two
 * unused arrays) -- then x_iso_scale loc / s [nt] (SoftplusNormal; prior HalfCauchy(0, 1), :1110-1112) and x_iso loc / s
 * [S][nt] (prior Normal(x_iso_loc, x_iso_scale), :1114-1116).  Noise appended to the noise vector: 2 globals, five [F][P]
 * arrays, bias [P], (unused [P]), x_iso_scale [nt], x_iso [S][nt].  One GPU only. */
polee_status polee_regression_set_joint_likelihood(polee_regression *reg, polee_approx *ap, const int32_t *gene_of,
                                                   const float *x_isoform_init, int32_t num_splice_features,
                                                   const int32_t *pair_transcript, const int32_t *pair_feature,
                                                   int64_t num_pairs);
/* Adam's learning rate of polee_regression_fit (default 2e-3: models/polee_regression.py:326; the joint model sets 1e-3) */
polee_status polee_regression_set_learning_rate(polee_regression *reg, float learning_rate);
int64_t polee_regression_num_isoform_params(const polee_regression *reg);
polee_status polee_regression_get_isoform_params(polee_regression *reg, float *params);
polee_status polee_regression_set_isoform_params(polee_regression *reg, const float *params);
/* gradient of the isoform block left by the last polee_regression_eval */
polee_status polee_regression_get_isoform_grad(polee_regression *reg, float *grad);
/* Samples sharded over ranks: every rank creates the model over ITS samples (S = local count, the
 * same F, n, hinges, x_init_mean and seed everywhere), so the shared parameters are replicas and qx_* are local.
 * Per step one sum all-reduce of (F+2) n + 32 f32 observation-model statistics is the only exchange. */
polee_status polee_regression_set_comm(polee_regression *reg, polee_comm *comm_or_null);
/* kernel_regression_weights (src/polee.py:36-47) as the model uses them: f32 [degree][n] */
polee_status polee_regression_weights(polee_regression *reg, float *weights);
/* loss and (optionally) its gradient w.r.t. the flat parameter vector at the current parameters, for the draw
 * defined by `noise` (host, num_noise values) or, when NULL, by the device RNG with `seed`; no update. */
polee_status polee_regression_eval(polee_regression *reg, const float *noise_or_null, uint64_t seed, float *loss,
                                   float *grad_or_null);
/* classify (models/polee_regression.py:342-413): the design matrix of the (testing) samples is a latent variable -- a relaxed one-hot
 * row per sample whose logits are the only new trainable quantity -- while everything the fitted model shares stays fixed.  The
 * host side (polee_amd/regression.py, RNASeqLinearRegression.classify; the Julia caller models/classify.jl does the same through
 * PyCall) draws the relaxed rows and owns the logits; the device model over the testing samples provides:
 *   _set_design     the step's design matrix, f32 [S][F] (replaces the one given at creation; from then on every evaluation also
 *                   computes d loss / d design -- the observation model's term, -sum_j a[s][j] w_eff[f][j]);
 *   _set_trainable  Adam of polee_regression_fit moves the flat parameters [begin, end) only (the testing samples' qx_loc /
 *                   qx_softplus_scale blocks; begin == end with point estimates); default: all of them;
 *   _design_grad    d loss / d design of the last evaluation or fit step, f32 [S][F].
 * Transcript-level model on one GPU (the gene-level classify, :601-651, is not built). */
polee_status polee_regression_set_design(polee_regression *reg, const float *design);
polee_status polee_regression_set_trainable(polee_regression *reg, int64_t begin, int64_t end);
polee_status polee_regression_design_grad(polee_regression *reg, float *grad);
/* Latent design (RNASeqPCA, models/polee_pca.py:14-92): the design matrix is a trained parameter z [S][F] (F = the latent
 * dimensionality, fixed at creation: at most 16) with a Normal(0, prior_scale) prior (latent_space_model_fn, :52-56) and a point
 * (Deterministic) surrogate (:58-59), so every evaluation adds -log p(z) = sum z^2 / (2 sigma^2) + log sigma + log(2 pi) / 2 to the
 * loss (polee_regression_eval and the loss trace), and polee_regression_fit trains z with an Adam of its own (the same constants,
 * step clock and rate as the flat parameters; polee_regression_set_trainable does not govern it) inside the step: no host work
 * between steps.
 *   _set_latent_design  uploads z0, f32 [S][F], zeroes z's Adam moments and turns the mode on; prior_scale must be positive and
 *                       finite.  Transcript-level model on one GPU, with a likelihood handle or point estimates (the conditions of
 *                       polee_regression_set_design; anything else POLEE_ERR_UNSUPPORTED).
 *                       (F is fixed by polee_regression_create, which refuses more than 16 factors with POLEE_ERR_UNSUPPORTED.)
 *   _get_design         the current design matrix (z on a latent handle), f32 [S][F].
 * On a latent handle polee_regression_set_design replaces z and leaves its moments alone, and polee_regression_design_grad returns
 * the TOTAL d loss / dz, prior term z / sigma^2 included (on other handles: the observation model's term, as above). */
polee_status polee_regression_set_latent_design(polee_regression *reg, const float *z0, float prior_scale);
polee_status polee_regression_get_design(polee_regression *reg, float *design);
/* niter steps of fit() (models/polee_regression.py:303-340): draw, loss + gradient, Adam(2e-3, 0.9, 0.999, 1e-7).
 * noise (optional, tests): host [niter][num_noise].  loss_trace (optional): f32 [niter]. */
polee_status polee_regression_fit(polee_regression *reg, int32_t niter, uint64_t seed, const float *noise_or_null,
                                  float *loss_trace_or_null);

/* ---- construction of the likelihood matrix (first slice) ------------------------------------
 * Replaces, for pre-parsed inputs, the reference's intersection of alignment pairs with transcripts and the
 * conditional fragment probabilities of its SimplisticFragModel (bias terms = 1):
 *   parallel_intersection_loop (src/rnaseq_sample.jl:58-121), fragmentlength (src/transcripts.jl:273-446),
 *   effective_length / condfragprob (src/fragmodel.jl:119-169), sortperm + compact_indexes! + sparse
 *   (src/rnaseq_sample.jl:126-157, 470-489).
 * BAM / GFF parsing stays upstream; the fragment model is estimated here from the alignment pairs themselves
 * (polee_fragmodel_estimate, polee_read_assign, below) and the bias model trained from the assigned fragments
 * (polee_bias_train_*).  Coordinates are 1-based inclusive.
 *   transcripts  j = 0..n-1 (= t.metadata.id - 1): sequence id, strand (+1 / -1), exons ascending and disjoint
 *   fragments    i = 0..m-1 = alignment pairs: sequence id, strand, the LEFTMOST mate (m1) and, for paired-end reads,
 *                the other one (m2; m2_left == 0: single-end); per mate its CIGAR as (operation code, length) pairs
 *                in BAM coding (0 M, 1 I, 2 D, 3 N, 4 S), cig?_ptr[i] .. cig?_ptr[i+1] into cig_op / cig_len (an
 *                empty range = one match over [left, right]); m1_is_flag16: the lone mate's SAM flag is exactly 16
 *                (the reference's test `aln.flag == SAM.FLAG_REVERSE != 0`, src/fragmodel.jl:130)
 *   fragmodel    fraglen_pmf / fraglen_cdf f32 [2000] (index l-1 holds length l), the median, strand specificity,
 *                alt_frag_model (src/fragmodel.jl:23-115)
 * Result: X's rows compressed (what polee_loglik_create_from_xt takes): tcolptr u64 [rows+1] 1-based, trowval u32
 * 1-based transcript ids ascending within a row, tnzval f32; effective_lengths f32 [n]; row_fragment i64 [rows] =
 * the fragment of every row (fragments compatible with no transcript are dropped, as compact_indexes! does; rows keep
 * the fragments' input order -- the reference numbers them in the order of its interval trees, a permutation the
 * likelihood does not see). */
typedef struct {
    int32_t n;
    const int32_t *seq;
    const int8_t *strand;
    const int64_t *exon_ptr;   /* [n+1] */
    const int64_t *exon_first, *exon_last;
} polee_xb_transcripts;
typedef struct {
    int64_t m;
    const int32_t *seq;
    const int8_t *strand;
    const int64_t *m1_left, *m1_right, *m2_left, *m2_right;
    const uint8_t *m1_is_flag16;
    const int64_t *cig1_ptr, *cig2_ptr;  /* [m+1] each */
    const uint8_t *cig_op;
    const int32_t *cig_len;
} polee_xb_fragments;
typedef struct {
    const float *fraglen_pmf, *fraglen_cdf;
    int32_t fraglen_median;
    float strand_specificity;
    int32_t alt_frag_model;
} polee_xb_fragmodel;
/* A TRAINED bias model for the reference's default BiasedFragModel (src/fragmodel.jl:174-445; training, src/bias.jl:266-786:
 * polee_bias_train_* below -- what still comes from upstream are the training fragments themselves).  tseq: the transcripts' spliced sequences in transcript orientation (t.metadata.seq), one code per base:
 * 0 A, 1 C, 2 G, 3 T, 4 anything else; tseq_ptr [n+1] (tseq_ptr[0] = 0, lengths = exonic lengths).  Sequence bias
 * (SeqBiasModel{:left} / {:right}, bias.jl:157-160, 419-456): seqbias_len = 20 positions, orders [20] (-1: position not in
 * the model), ps [20][4][ps_ctx] row-major (the reference's ps[i, c+1, ctx+1]), ps_ctx >= 4^(largest order).  gc_bins: the
 * SimpleHistogramModel's bins (bias.jl:459-521).  pos_terms [pos_maxtlen] + pos_p: PositionalBiasModel (bias.jl:523-659) or
 * NULL (use_pos_bias = false, the default).  high_prob_fraglens: the BIAS_EFFLEN_NUM_FRAGLENS most probable fragment lengths
 * in descending probability (fragmodel.jl:358-359).  m1_reverse [m]: the lone mate of a single-end fragment has
 * FLAG_REVERSE set (transcripts.jl:486); may be NULL when every fragment is paired.
 * Not reproducible: context positions beyond a transcript's ends are RANDOM nucleotides in the reference (bias.jl:83-85,
 * 424-429); here they read as A. */
typedef struct {
    const int64_t *tseq_ptr;
    const uint8_t *tseq;
    int32_t seqbias_len, ps_ctx;
    const int32_t *orders_left, *orders_right;
    const float *ps_left, *ps_right;
    int32_t gc_nbins;
    const float *gc_bins;
    double pos_p;
    const double *pos_terms;
    int32_t pos_maxtlen;
    int32_t num_fraglens;
    const int32_t *high_prob_fraglens;
    const uint8_t *m1_reverse;
} polee_xb_biasmodel;
typedef struct polee_xbuild polee_xbuild;
polee_status polee_xbuild_run(polee_ctx *ctx, const polee_xb_transcripts *transcripts, const polee_xb_fragments *fragments,
                              const polee_xb_fragmodel *fragmodel, polee_xbuild **out);
/* The same under the BiasedFragModel: compute_transcript_bias! (bias.jl:834-858), effective_length (fragmodel.jl:372-410),
 * condfragprob with genomic_to_transcriptomic (fragmodel.jl:413-445, transcripts.jl:452-538).  polee_xbuild_get_bias
 * returns the transcripts' bias vectors (left / right f32 [tseq_ptr[n]], laid out like tseq) and the kernel's time. */
polee_status polee_xbuild_run_biased(polee_ctx *ctx, const polee_xb_transcripts *transcripts, const polee_xb_fragments *fragments,
                                     const polee_xb_fragmodel *fragmodel, const polee_xb_biasmodel *biasmodel, polee_xbuild **out);
polee_status polee_xbuild_get_bias(const polee_xbuild *xb, float *left_bias_or_null, float *right_bias_or_null, double *ms_bias_or_null);
void polee_xbuild_destroy(polee_xbuild *xb);
/* rows and non-zeros of the result; kernel times (ms): effective lengths, counting pass, filling pass */
polee_status polee_xbuild_sizes(const polee_xbuild *xb, int64_t *rows, int64_t *nnz, double *ms_efflen, double *ms_count,
                                double *ms_fill);
/* copies the result to host arrays (any pointer may be NULL) */
polee_status polee_xbuild_get(const polee_xbuild *xb, uint64_t *tcolptr, uint32_t *trowval, float *tnzval,
                              float *effective_lengths, int64_t *row_fragment);
/* X (by columns, 1-based: polee_loglik_create's arguments) uploaded ONCE for the two device builders that read it when a sample is
 * prepared from host arrays -- the tree (PolyaTreeTransform(X, :cluster), ptt.jl:35-52 -> hclust.jl:180-330) and the layout
 * (RNASeqSample, likelihood.jl:2-41's X).  polee_loglik_create + polee_hclust_parallel_device each upload their own copy: 2.9 GB over
 * PCIe at C2 instead of 1.9 GB.  The handle may be used from two contexts of the same device at once (the builders only read it) and
 * must outlive both calls.  POLEE_ERR_UNSUPPORTED when rows or non-zeros need more than 32 bits (the host paths take those). */
typedef struct polee_devx polee_devx;
polee_status polee_devx_upload(polee_ctx *ctx, int64_t m, int64_t n, const void *colptr, int colptr_bytes, const uint32_t *rowval,
                               const float *nzval, polee_devx **out);
/* nzval may be NULL in polee_devx_upload and follow here: the tree needs colptr + rowval only and can start while the values are on
 * their way (what sample_and_tree of the Python mirror does) */
polee_status polee_devx_upload_values(polee_devx *dx, const float *nzval);
void polee_devx_destroy(polee_devx *dx);
/* as polee_loglik_create / polee_hclust_parallel_device on the arrays the handle was made from: the same layout byte for byte, the same tree.
 * nzval_or_null: the values, if the handle has none yet -- they go up beside the layout's first kernels (row keys, sort, column search
 * need colptr + rowval only) and stay in the handle: at most ONE call that passes values may run on a handle at a time (the
 * handle's value buffer is written by it; calls on a handle that already holds its values only read it and may run side by side).
 * With the device layout builder switched off (POLEE_DEVICE_BUILD=0 or a host-builder knob) the layout is built on the host from
 * the handle's arrays, as polee_loglik_create would. */
polee_status polee_loglik_create_from_devx(polee_ctx *ctx, polee_devx *dx, const float *nzval_or_null, const int64_t *ks_or_null, polee_loglik **out);
polee_status polee_hclust_parallel_device_from_devx(polee_ctx *ctx, const polee_devx *dx, int32_t *node_parent_idxs, int32_t *node_js);
/* The likelihood handle straight from an xbuild result, without X leaving the device: rows_to_device -> layout kernels
 * (as polee_loglik_create_from_xt on polee_xbuild_get's arrays; ks_or_null: host array [rows]).  The xbuild handle stays valid. */
polee_status polee_loglik_create_from_xbuild(polee_ctx *ctx, const polee_xbuild *xb, const int64_t *ks_or_null, polee_loglik **out);
/* ... and the tree (polee_hclust_parallel_device) from the same result on the device: alignments -> X -> tree + layout -> fit
 * without X visiting the host (the columns of X by a stable sort of the result's rows by transcript). */
polee_status polee_hclust_parallel_device_from_xbuild(polee_ctx *ctx, const polee_xbuild *xb, int32_t *node_parent_idxs, int32_t *node_js);

/* ---- the fragment model from the alignment pairs themselves ------------------------------------------
 * A fragment is one alignment pair of one read (there are no read ids: one pair is one read).
 *
 * polee_fragmodel_estimate: the counts of SimplisticFragModel(rs, ts) (src/fragmodel.jl:35-67).  Over every (transcript, fragment)
 * pair of the same sequence whose transcript contains the fragment's span and is compatible with it (fragmentlength is not
 * nothing): counts[0] = such pairs, counts[1] = pairs of equal strands, counts[2] = pairs whose fragment has the other of +1 / -1
 * (any other fragment strand is STRAND_BOTH: neither); per fragment the MINIMUM of its positive lengths (the reference keys that
 * minimum by hash(alnpr): here the pair itself); counts[3] = fragments whose minimum is above 2000, hist[l-1] = fragments whose
 * minimum is l <= 2000, min_fraglen[i] = the minimum (0: none; host array [m] or NULL).  Integer reductions only: the result does
 * not depend on scheduling.  The pmf / cdf / median and the strand specificity are host arithmetic on these (polee_amd/fragmodel.py). */
polee_status polee_fragmodel_estimate(polee_ctx *ctx, const polee_xb_transcripts *transcripts, const polee_xb_fragments *fragments,
                                      int64_t *counts, int64_t *hist, int64_t *min_fraglen_or_null);
/* polee_read_assign: one transcript per row of an xbuild result (= per read) and the fragment's interval on it
 * (src/rnaseq_sample.jl:346-373, genomic_to_transcriptomic src/transcripts.jl:452-517, src/fragmodel.jl:205-246).  transcripts /
 * fragments: what xb was built from.  tseq_ptr [n+1]: the transcripts' lengths (tseq_ptr[0] = 0, lengths = exonic lengths).
 * m1_reverse [m]: as in polee_xb_biasmodel (NULL only when every fragment is paired).  xs [n]: the mixture.
 * mode 0, the draw: z_sum = the f64 sum, in the row's order, of the f32 products xs[j] * nzval; r = the 53-bit uniform of words
 * 0, 1 of the Philox block (key seed, counter (low word of i, high word of i, 0, 0x66617373 'fass'), i = the row's fragment); the
 * entries in ascending transcript order with zj = product / z_sum: the first zj > r is taken, otherwise r -= zj; the last entry
 * takes what is left.  mode 1, as the reference is written (its loop has no break and its condition holds at the last entry):
 * the LAST entry of every row; xs (may be NULL) and seed are not used.
 * Outputs, host arrays [rows of xb]: transcript (0-based), tpos (1-based, transcript orientation) and fraglen of
 * genomic_to_transcriptomic(t, rs, alnpr, fallback_fraglen) -- an empty interval is tpos = 0, fraglen = 0 --, flags: bit 0 the
 * pair has both mates (its length was observed, not guessed), bit 1 strand match, bit 2 strand mismatch (bits 1, 2 only with a
 * non-empty interval). */
polee_status polee_read_assign(polee_ctx *ctx, const polee_xbuild *xb, const polee_xb_transcripts *transcripts,
                               const polee_xb_fragments *fragments, const int64_t *tseq_ptr, const uint8_t *m1_reverse_or_null,
                               const float *xs, uint64_t seed, int32_t mode, int32_t fallback_fraglen, int32_t *transcript,
                               int64_t *tpos, int32_t *fraglen, uint8_t *flags);

/* ---- Gibbs sampler of the exact posterior (src/gibbs.jl; `polee debug-sample`, src/main.jl:925-957) -----------------------------
 * Collapsed Gibbs sampling over fragment assignments: draws of the transcript mixture from p(y | X) under a Dirichlet(1) prior,
 * num_chains (1..32) chains at once (csrc/gibbs.hip).  X as polee_loglik_create takes it (or fragment-major, _from_xt:
 * the same layout); efflens_or_null: effective lengths (> 0), NULL = --no-efflen.  Every chain starts from Gamma(1) draws of its own.
 * A sweep = one assignment of every fragment + one draw of the mixture, two kernel launches; polee_gibbs_run only queues them.
 * Randomness: Philox4x32-10 keyed by (seed, sweep, chain, original fragment / transcript), sweeps numbered 1, 2, ... from creation:
 * a chain's draws depend on (X, seed, chain index) only -- not on the number of chains -- and are bitwise reproducible. */
typedef struct polee_gibbs polee_gibbs;
polee_status polee_gibbs_create(polee_ctx *ctx, int64_t m, int64_t n, const void *colptr, int colptr_bytes, const uint32_t *rowval,
                                const float *nzval, const float *efflens_or_null, int32_t num_chains, uint64_t seed, polee_gibbs **out);
/* X given fragment-major (tcolptr [m+1] uint64 1-based, trowval 1-based: polee_loglik_create_from_xt's arguments) */
polee_status polee_gibbs_create_from_xt(polee_ctx *ctx, int64_t m, int64_t n, const uint64_t *tcolptr, const uint32_t *trowval,
                                        const float *tnzval, const float *efflens_or_null, int32_t num_chains, uint64_t seed,
                                        polee_gibbs **out);
void polee_gibbs_destroy(polee_gibbs *g);
/* the chains' mixture state, unnormalised: g0 f32 [C][n] (finite, >= 0), or NULL = fresh Gamma(1) draws */
polee_status polee_gibbs_set_state(polee_gibbs *g, const float *g0_or_null);
/* room for draws_per_chain stored draws per chain (f32 [C][draws][n] on the device); empties the store */
polee_status polee_gibbs_reserve(polee_gibbs *g, int32_t draws_per_chain);
/* nsweeps sweeps; stride > 0: the state after every stride-th sweep is stored (x_j = (g_j / l_j) / sum_k g_k / l_k), counted
 * across calls with the same stride; stride 0 = burn-in, nothing stored.  Asynchronous: polee_gibbs_sync waits. */
polee_status polee_gibbs_run(polee_gibbs *g, int32_t nsweeps, int32_t stride);
/* waits for the queued sweeps; POLEE_ERR_NONFINITE if a mixture draw was not finite and positive */
polee_status polee_gibbs_sync(polee_gibbs *g);
polee_status polee_gibbs_num_stored(const polee_gibbs *g, int32_t *draws_per_chain);
/* stored draws [first, first + count) of every chain -> out f32 [C][count][n] */
polee_status polee_gibbs_get_draws(polee_gibbs *g, int32_t first, int32_t count, float *out);
/* fragments per transcript in the last sweep, single-transcript fragments included -> counts u32 [C][n] */
polee_status polee_gibbs_get_counts(polee_gibbs *g, uint32_t *counts);
/* split-R-hat per transcript over all stored draws (convergence_stats, gibbs.jl:283-319) -> rhat f32 [n] */
polee_status polee_gibbs_rhat(polee_gibbs *g, float *rhat);
typedef struct {
    int64_t m, n, nnz;
    int32_t num_chains;
    int64_t num_multi_rows;   /* fragments sampled every sweep (two or more compatible transcripts)          */
    int64_t num_single_rows;  /* fragments with one compatible transcript: a constant count per transcript     */
    int64_t num_empty_rows;   /* fragments with none: dropped (gibbs.jl:202-211 never counts them)            */
    int64_t multi_nnz;        /* non-zeros a sweep reads                                                      */
    int64_t num_tiles;        /* workgroups of the assignment kernel                                          */
    int32_t rows_per_tile;
    int64_t sweeps_done;      /* sweeps run since creation (the next sweep is number sweeps_done + 1)         */
} polee_gibbs_info;
polee_status polee_gibbs_get_info(const polee_gibbs *g, polee_gibbs_info *info);

/* ---- EM maximum-likelihood estimate (src/em.jl:3-87; `polee debug-optimize`, src/main.jl:960-988) -------------------------------
 * expectation_maximization: the mixture y that maximises sum_i ks_i log sum_j X_ij y_j, by y_j <- y_j g_j / M with g the gradient
 * of a likelihood pass and M = the sum of ks over the non-empty fragments (csrc/em.hip).  The handle works on an
 * existing polee_loglik -- X is neither uploaded nor laid out again -- and keeps it alive.  An iteration is one K = 1 likelihood
 * pass and one small launch; mixture, log-likelihood trace and stop rule stay on the device.
 * An EM handle uses its loglik's ONE evaluation slot (see polee_loglik_eval): while polee_em_create / _reset with a y0 that has
 * zeros, polee_em_run, or iterations it queued are in flight, nothing else -- polee_loglik_eval, a polee_vi or polee_regression step,
 * another polee_em -- may evaluate the same polee_loglik.  With polee_loglik_set_deterministic(ll, 1) a run is bitwise
 * reproducible. */
typedef struct polee_em polee_em;
/* y0_or_null: the start, f32 [n], finite, >= 0, with a positive sum (normalised on entry); NULL = 1/n (em.jl:22).  A y0 that is 0
 * on every transcript some fragment is compatible with would give that fragment probability 0: POLEE_ERR_BAD_ARG, from
 * polee_em_reset too (single-transcript fragments are checked against the layout's per-transcript counts; for the others a y0
 * with zeros costs two likelihood passes, which count the fragments the pass does not skip). */
polee_status polee_em_create(polee_loglik *ll, const float *y0_or_null, polee_em **out);
void polee_em_destroy(polee_em *em);
/* back to iteration 0 at a new start (as polee_em_create's); the trace is emptied */
polee_status polee_em_reset(polee_em *em, const float *y0_or_null);
/* Up to max_iters more iterations (em.jl:41-79).  Stop rule, em.jl:76: the run ends with the first iterate whose log-likelihood
 * exceeds the previous one's by less than tol (the reference: 1e-6); tol < 0 switches the rule off, the call then makes exactly
 * max_iters iterations.  lp is summed in f64 here (Float32 in the reference, which therefore stops at the first increase its sum
 * cannot represent).  check_every >= 1 iterations are queued between two reads of the device's stop flag; once stopped the
 * mixture is frozen, so the iterations queued behind the stop change nothing, and further calls return at once whatever their
 * tol: to go on from there, polee_em_reset(em, the mixture polee_em_get_mixture returns), which empties the trace.  Returns after
 * the last queued iteration has run; POLEE_ERR_NONFINITE when an iterate's log-likelihood is not finite. */
polee_status polee_em_run(polee_em *em, int32_t max_iters, double tol, int32_t check_every);
/* waits for the context's stream; POLEE_ERR_NONFINITE as polee_em_run */
polee_status polee_em_sync(polee_em *em);
/* the current iterate, normalised: y f32 [n], sums to 1 to f32 rounding */
polee_status polee_em_get_mixture(polee_em *em, float *y);
/* 1e6 (y / efflens) / sum(y / efflens) (em.jl:82-84); efflens_or_null == NULL (--no-efflen): 1e6 y.  tpm f32 [n] */
polee_status polee_em_get_tpm(polee_em *em, const float *efflens_or_null, float *tpm);
/* lp of iterates 1, 2, ... (the reference's `@show lp`, em.jl:74): the first min(capacity, *count) into lp; *count = entries held */
polee_status polee_em_get_trace(polee_em *em, double *lp, int64_t capacity, int64_t *count);
typedef struct {
    int64_t n;
    int64_t M;             /* sum of ks over the non-empty fragments (their number without ks)                          */
    int64_t iters;         /* iterations made since creation / reset                                                      */
    int32_t converged;     /* the stop rule has fired                                                                     */
    int32_t nonfinite;     /* an iterate's log-likelihood was not finite                                                  */
    double lp_start;       /* log-likelihood of the start (NaN before the first run)                                      */
    double last_lp;        /* ... of the current iterate                                                                  */
    double last_increase;  /* ... minus the previous iterate's                                                            */
    double sum_y;          /* f64 sum of the iterate as the device holds it (1 up to f32 rounding)                        */
    double kkt_max;        /* compute_kkt != 0: the fixed-point residual max_j y_j |g_j(y) / M - 1| of the mixture that          */
                           /* polee_em_get_mixture hands out, from a gradient summed in f64 by a pass of its own over the       */
                           /* layout (2 ms at 30 M fragments); else -1                                                           */
} polee_em_info;
polee_status polee_em_get_info(polee_em *em, int compute_kkt, polee_em_info *info);

/* ---- the alternative approximations (`prep --approx-method`, src/main.jl:5-23; src/likelihood-approximation-alt.jl) ------------
 * The baselines the default approximation is judged against.  One handle runs the VI loop of a method on an existing polee_loglik,
 * which it keeps alive (csrc/altvi.hip): K draws per step through ONE sparse pass, the method's chain rule,
 * the reference's ADAM (likelihood-approximation.jl:107-146) on two parameter vectors of n - 1 values, no host synchronisation
 * inside polee_altvi_run.  None of the methods applies the effective-length Jacobian (they call log_likelihood directly).
 * Built: logistic_normal (likelihood-approximation-alt.jl:50-203), normal_ilr (:503-616, isometric_log_ratios.jl:43-128) and
 * normal_alr (:619-736, additive_log_ratios.jl:12-71); their parameters are mu, omega.  The two Polya-tree alternatives are named
 * here so that the numbering is the reference's list, and answered with POLEE_ERR_UNSUPPORTED.
 * Like polee_em, a handle uses its loglik's one evaluation slot while steps are in flight. */
enum {
    POLEE_ALT_LOGISTIC_NORMAL = 1,  /* LogisticNormalApprox                                   */
    POLEE_ALT_KUMARASWAMY_PTT = 2,  /* KumaraswamyPTTApprox (:331-498): not built             */
    POLEE_ALT_LOGIT_NORMAL_PTT = 3, /* LogitNormalPTTApprox (:208-328): not built             */
    POLEE_ALT_NORMAL_ILR = 4,       /* NormalILRApprox; needs a tree                          */
    POLEE_ALT_NORMAL_ALR = 5        /* NormalALRApprox                                        */
};
typedef struct polee_altvi polee_altvi;
typedef struct {
    int32_t method;              /* POLEE_ALT_*                                                                        */
    int32_t num_steps;           /* LIKAP_NUM_STEPS = 500                                                              */
    int32_t num_mc_samples;      /* LIKAP_NUM_MC_SAMPLES = 6 (1..8)                                                    */
    int32_t gradonly;            /* default 1: no ELBO / log-likelihood trace                                          */
    int32_t refidx;              /* normal_alr: 1-based reference element, -1 = n (likelihood-approximation-alt.jl:641) */
    int32_t reserved;
    uint64_t seed;               /* device Philox seed                                                                 */
    const float *z0;             /* optional HOST noise [num_steps][num_mc][n-1]; replaces the device RNG              */
    double eps;                  /* clamp of xs to [eps, 1 - eps], 1e-10 (:109, 133)                                   */
    double adam_initial_learning_rate, adam_learning_rate_decay, adam_min_learning_rate, adam_eps, adam_rv, adam_rm;
    double max_step0, max_step1; /* ss_max_*_step: 2e-2 for logistic_normal (:66-67), 2e-1 for ILR and ALR (:520-521, 637-638) */
} polee_altvi_opts;
/* the reference's constants of `method` */
void polee_altvi_default_opts(int32_t method, polee_altvi_opts *opts);
typedef struct {
    int32_t steps_done;
    int32_t nonfinite_step; /* first step with a non-finite gradient, 0 if none */
    double last_elbo;       /* !gradonly */
    double last_lp_mean;    /* !gradonly */
} polee_altvi_stats;
/* Initial values: mu = 0; omega = 0.1 for logistic_normal (:79 -- not log 0.1), log(0.1f0) for ILR and ALR (:536, 655).
 * t_or_null: the tree of normal_ilr (ILRTransform, isometric_log_ratios.jl:3-31), ignored by the other two. */
polee_status polee_altvi_create(polee_loglik *ll, polee_ptt *t_or_null, const polee_altvi_opts *opts, polee_altvi **out);
void polee_altvi_destroy(polee_altvi *a);
/* enqueues nsteps iterations on the context's stream without host synchronisation */
polee_status polee_altvi_run(polee_altvi *a, int32_t nsteps);
/* waits for the stream; POLEE_ERR_NONFINITE if a step met a non-finite gradient */
polee_status polee_altvi_sync(polee_altvi *a);
/* the two parameter vectors, f32 [n-1] each (mu, omega); either pointer may be NULL */
polee_status polee_altvi_get_params(polee_altvi *a, float *p0, float *p1);
polee_status polee_altvi_set_params(polee_altvi *a, const float *p0, const float *p1);
polee_status polee_altvi_get_stats(polee_altvi *a, polee_altvi_stats *stats);
/* !gradonly: per step the reference's elbo -- logistic_normal: the LAST draw's lp + ladj over K (an assignment in the draw loop,
 * :162, 180); ILR and ALR: the mean over the draws (:579, 698) -- and the mean log-likelihood.  Either pointer may be NULL. */
polee_status polee_altvi_get_trace(polee_altvi *a, double *elbo, double *lp_mean);
/* the noise of 1-based `step`: z0 f32 [K][n-1] */
polee_status polee_altvi_export_noise(polee_altvi *a, int32_t step, float *z0);
/* Test hook: the K draws of the NEXT step at the current parameters, nothing updated.  Any output may be NULL.  xs [K][n],
 * x_grad [K][n], y_grad [K][n-1], the two averaged parameter gradients [n-1], lp [K], ladj [K]. */
polee_status polee_altvi_eval_gradients(polee_altvi *a, float *xs, double *x_grad, double *y_grad, float *p0_grad, float *p1_grad,
                                        double *lp, double *ladj);
/* sample_likap (src/evaluate.jl:34-74, 203-275): `count` draws through the fit's forward kernels, each divided by the effective
 * lengths and renormalised; out f32 [count][n].  p0, p1 = mu, omega (sigma = exp(omega), for logistic_normal too, :37);
 * refidx as in polee_altvi_opts; z0_or_null: HOST noise [count][n-1]. */
polee_status polee_alt_sample(polee_ctx *ctx, int32_t method, polee_ptt *t_or_null, int32_t n, const float *p0, const float *p1,
                              const float *efflens, int32_t refidx, int32_t count, uint64_t seed, const float *z0_or_null, float *out);
/* a = sqrt(s / (r (r + s))), b = -sqrt(r / (s (r + s))) for r, s leaves below the left and right child of every internal node
 * (isometric_log_ratios.jl:62-66); ab f64 [count][2].  Host only. */
polee_status polee_ilr_coefficients(const int32_t *r, const int32_t *s, int64_t count, double *ab);

/* ---- `polee sample` (src/main.jl:239-289 flags, :756-919 handler) ----------------------------------------------------------------
 * A stream of draws from one fitted approximation with everything the command does after the draw: the effective-length adjustment
 * (xs ./= efflens; xs ./= sum(xs), main.jl:850-853), the running posterior mean (:857) and prop_to_counts (:859-880), on the device.
 * The raw draw with index d is bit for bit row d of polee_sampler_draw(..., ndraws > d, the same seed), for any split of the draws
 * into polee_sampler_next calls.  Arithmetic (csrc/sample.hip): t_j = x_j / l_j in f32; S = sum t_j in f64;
 * prop_j = (float)((double)t_j / S); the posterior mean is accumulated in f64 per transcript in draw order and handed out as f32;
 * expected counts in f64: e_j = (double)prop_j l_j, counts_j = e_j / sum(e) m. */
typedef struct polee_sampler polee_sampler;
/* t: a single tree; mu, sigma, alpha f32 [n-1] (sigma = exp(omega)); efflens f32 [n], positive and finite; 0 <= m < 2^31.
 * Parameters, effective lengths and all work buffers live on the device; the handle keeps the tree alive and uses its scratch. */
polee_status polee_sampler_create(polee_ptt *t, const float *mu, const float *sigma, const float *alpha, const float *efflens,
                                  int64_t m, uint64_t seed, polee_sampler **out);
void polee_sampler_destroy(polee_sampler *s);
/* The next `count` draws (the draw index continues from the previous call).  z0_or_null: f32 [count][n-1], the N(0,1) noise of these
 * draws, or NULL = the device RNG.  Outputs, each optional, one download each: raw f32 [count][n] (the draws as polee_sampler_draw
 * gives them), props f32 [count][n], counts f64 [count][n] = prop_to_counts of every row -- count_mode 0: expected_counts
 * (main.jl:859-863); 1: sampled counts (--sample-counts): an exact multinomial draw of m reads with shares e_j, integers, every row
 * sums to m, a pure function of (the draw, m, seed, draw index); see polee_multinomial_counts.  The posterior mean is accumulated
 * whatever is asked for. */
polee_status polee_sampler_next(polee_sampler *s, int32_t count, int32_t count_mode, const float *z0_or_null, float *raw_or_null,
                                float *props_or_null, double *counts_or_null);
/* draws made so far */
polee_status polee_sampler_num_draws(polee_sampler *s, int64_t *ndraws);
/* post_mean f32 [n]: the mean of all props so far; est_counts f64 [n] = prop_to_counts(post_mean) under count_mode (mode 1 draws
 * under the draw index 2^64 - 1). */
polee_status polee_sampler_mean(polee_sampler *s, float *post_mean, double *est_counts_or_null, int32_t count_mode);
/* D exact multinomial draws of m items over n categories: p f64 [D][n], shares >= 0 and finite, need not be normalised; counts u32
 * [D][n], every row sums to m.  0 <= m < 2^31, 1 <= n <= 2^30.  Row r is draw first_draw + r: a pure function of (its shares, m,
 * seed, draw index) -- bitwise reproducible, independent of D and of how rows are batched.  Construction: m is split down a
 * balanced binary tree over the categories, Binomial(c, mass of the left half / mass of the node) at every node (n - 1 variates
 * per draw, whatever m is), exact binomial variates from counter-based Philox noise (csrc/binomial.hpp).  POLEE_ERR_BAD_ARG: a
 * negative or non-finite share, a row that sums to 0 with m > 0, sizes out of range.  POLEE_ERR_NONFINITE (here and from the
 * handle): a variate used up its fixed number of rejection attempts, which finite shares do not do. */
polee_status polee_multinomial_counts(polee_ctx *ctx, const double *p, int32_t D, int64_t n, int64_t m, uint64_t seed,
                                      uint64_t first_draw, uint32_t *counts);

/* ---- `polee model classify` (models/classify.jl, models/polee_classify.py:13-114; csrc/classify.hip) ------
 * RNASeqLogisticRegression: a multinomial logistic regression on log expression.  Parameters w [n][k], x_bias [n], z_bias [k], all
 * zero at creation (:18-20) and all trained.  logits = (x - x_bias) w + z_bias;
 *   loss = loss_scale sum_s CE(labels_s, softmax(logits_s)) + l1_penalty sum |w|          (:22-41; the penalty is not scaled)
 * and with an approximation handle the mean of that loss over draws_per_step draws x = log(sampler draw) (loss_sample, :43-49), so the
 * penalty counts once; no gradient flows through the sampler.  The penalty's gradient is l1_penalty sign(w), sign(0) = 0 (tf.abs).
 * The draws never leave the device; all sums have a fixed order (no float atomics): every result is bitwise reproducible.
 * Draw rule: the draw with index i uses seed + 0x9E3779B97F4A7C15 i (as polee_approx_feature_moments).  In polee_classify_fit,
 * i = (t - 1) D + d for draw d of Adam step t, D = draws_per_step, and t is the handle's step clock, which runs on across calls:
 * fit(2) then fit(3) equals fit(5).  polee_classify_eval and polee_classify_predict use i = their own draw number.
 * Every `ap` must live on the handle's context and have its n (else POLEE_ERR_BAD_ARG); S is the approximation's.  Label rows must be
 * one-hot (else POLEE_ERR_BAD_ARG).  On the point paths x [S][n] is log expression already and must be finite: POLEE_ERR_NONFINITE
 * otherwise (the reference takes log 0 silently when a TPM is 0 and no pseudocount is given, classify.jl:141-147). */
typedef struct polee_classify polee_classify;
typedef struct {
    int32_t draws_per_step; /* samples_per_iter, 5 (polee_classify.py:51) */
    float learning_rate;    /* 1e-4 (:69, :92) */
    float l1_penalty;       /* 1e-3 (:29-30) */
    float loss_scale;       /* 1 (:22) */
    float beta1, beta2, epsilon; /* tf.optimizers.Adam: 0.9, 0.999, 1e-7 */
} polee_classify_opts;
void polee_classify_default_opts(polee_classify_opts *opts);
/* 2 <= k <= 16, anything else POLEE_ERR_UNSUPPORTED; opts NULL = the defaults (polee_classify.py:14-20) */
polee_status polee_classify_create(polee_ctx *ctx, int32_t n, int32_t k, const polee_classify_opts *opts, polee_classify **out);
void polee_classify_destroy(polee_classify *cl);
/* new options from the next call on (fit's loss_scale, :74; fit_sample's samples_per_iter, :51); moments and clock stay */
polee_status polee_classify_set_opts(polee_classify *cl, const polee_classify_opts *opts);
/* w f32 [n][k], x_bias f32 [n], z_bias f32 [k] (get: each may be NULL); set leaves the Adam moments and the step clock alone */
polee_status polee_classify_get_params(polee_classify *cl, float *w, float *x_bias, float *z_bias);
polee_status polee_classify_set_params(polee_classify *cl, const float *w, const float *x_bias, const float *z_bias);
/* Adam moments and step clock back to zero (a fresh tf.optimizers.Adam, :66-70) */
polee_status polee_classify_reset(polee_classify *cl);
/* x_bias <- the column mean over samples of the log of ONE draw (:52-55); z0_or_null f32 [S][n-1]: the draw's N(0,1) noise */
polee_status polee_classify_init_bias(polee_classify *cl, polee_approx *ap, const float *z0_or_null, uint64_t seed);
/* x_bias <- the column mean of x f32 [S][n] (:75) */
polee_status polee_classify_init_bias_points(polee_classify *cl, const float *x, int32_t S);
/* loss_sample (:43-49) and its gradient, penalty term included, no update: exactly the numbers a fit step feeds to Adam (the same
 * kernels in the same order).  labels f32 [S][k]; z0_or_null f32 [D][S][n-1]; g_w [n][k], g_x_bias [n], g_z_bias [k], each may be NULL */
polee_status polee_classify_eval(polee_classify *cl, polee_approx *ap, const float *labels, const float *z0_or_null, uint64_t seed,
                                 float *loss, float *g_w, float *g_x_bias, float *g_z_bias);
/* loss (:22-41) on a fixed x f32 [S][n] */
polee_status polee_classify_eval_points(polee_classify *cl, const float *x, int32_t S, const float *labels, float *loss, float *g_w,
                                        float *g_x_bias, float *g_z_bias);
/* niter Adam steps on fresh draws (fit_sample :57-72, without the bias initialisation: polee_classify_init_bias); lr_t = lr
 * sqrt(1 - beta2^t) / (1 - beta1^t), p -= lr_t m / (sqrt(v) + epsilon).  z0_or_null f32 [niter][D][S][n-1], uploaded once;
 * loss_trace_or_null f32 [niter].  Nothing waits for the device until the last step is queued.  A call that fails partway keeps
 * the updates of the steps it completed, advances the clock by those, and leaves the accumulators at zero. */
polee_status polee_classify_fit(polee_classify *cl, polee_approx *ap, const float *labels, int32_t niter, uint64_t seed,
                                const float *z0_or_null, float *loss_trace_or_null);
/* fit (:74-95) on a fixed x, without the bias initialisation (polee_classify_init_bias_points) */
polee_status polee_classify_fit_points(polee_classify *cl, const float *x, int32_t S, const float *labels, int32_t niter,
                                       float *loss_trace_or_null);
/* predict_sample (:105-111): the mean over ndraws draws of softmax(logits), accumulated in f64; z0_or_null f32 [ndraws][S][n-1];
 * probs f32 [S][k] */
polee_status polee_classify_predict(polee_classify *cl, polee_approx *ap, int32_t ndraws, uint64_t seed, const float *z0_or_null,
                                    float *probs);
/* predict (:113-114) */
polee_status polee_classify_predict_points(polee_classify *cl, const float *x, int32_t S, float *probs);

/* ---- isoform effect sizes of `polee model regression --feature gene-isoform` (estimate_isoform_effect_sizes,
 * src/regression.jl:761-945; csrc/effects.hip) -------------------------------------------------------------
 * niter Monte-Carlo draws of the isoform bias x_j = zx qx_bias_scale_j + qx_bias_loc_j and of every factor's isoform coefficients
 * w_ij = zw qw_scale_ij + qw_loc_ij; per draw e_ij = log softmax_g(x + w_i)_j - log softmax_g(x)_j over the transcripts of j's gene
 * and a_ig = the Aitchison distance of the two compositions of gene g (= the population standard deviation of w_i over the gene).
 * Over the draws: mean = the mean of e; prob_de = #{e > effect_size} / niter, ONE-SIDED as the reference computes it (:850);
 * min = the k-th smallest |e|, k = clamp(round-half-even(target_coverage niter), 1, niter) (:912-915), exact.  The gene arrays are
 * the same over a, with aitchison_prob_de = #{|a| > aitchison_effect_size} / niter (:899).  A NaN threshold: that prob_de is not
 * computed and comes back as zeros.  Evaluated in log space with a max-subtracted log-sum-exp: finite where the reference's
 * exp / normalise / log underflows (a gene whose x spans more than ~700).  A gene of one isoform gives exact zeros; a gene without
 * transcripts gives zero distances.
 * Noise: Philox4x32-10 keyed by `seed`, counter (transcript, draw, stream / 4), stream 0 = x, 1 + i = w_i: a result depends on
 * (seed, inputs) alone, bit for bit, on any launch geometry; no float atomics.  zx_or_null f32 [niter][n] and zw_or_null f32
 * [niter][F][n] replace it (both or neither; zx_len / zw_len are their element counts and must be exactly niter n and niter F n).
 * POLEE_ERR_BAD_ARG: gene_of outside 0 .. G-1, niter < 1, target_coverage outside (0, 1], noise of the wrong size;
 * POLEE_ERR_UNSUPPORTED: niter > 4096 (28 bytes of LDS per draw). */
typedef struct polee_effects polee_effects;
/* gene_of i32 [n], 0-based, in any order: the transcripts are segmented by gene once, here */
polee_status polee_effects_create(polee_ctx *ctx, int32_t n, int32_t G, const int32_t *gene_of, int32_t F, polee_effects **out);
void polee_effects_destroy(polee_effects *fx);
/* qw_loc, qw_scale f32 [F][n]; qx_bias_loc, qx_bias_scale f32 [n]; outputs f32 [F][n] (three) and f32 [F][G] (three);
 * kernel_ms_or_null: the kernel's time between two events on the context's stream */
polee_status polee_effects_run(polee_effects *fx, const float *qw_loc, const float *qw_scale, const float *qx_bias_loc,
                               const float *qx_bias_scale, int32_t niter, double target_coverage, double effect_size_or_nan,
                               double aitchison_effect_size_or_nan, uint64_t seed, const float *zx_or_null, int64_t zx_len,
                               const float *zw_or_null, int64_t zw_len, float *min_effect_sizes, float *mean_effect_sizes, float *prob_de,
                               float *aitchison_min, float *aitchison_mean, float *aitchison_prob_de, double *kernel_ms_or_null);

/* ---- `polee model tsne` (models/tsne.jl:52-99, models/polee_tsne.py:17-185, :213-398; csrc/tsne.hip) -------
 * Parametric t-SNE of log expression: z = lx W, W f32 [n][C], zero at creation (the caller sets W0, :293-298); lx = log of one draw
 * per sample from the fitted approximations, drawn afresh at every evaluation, no gradient through it; with the *_points entries
 * lx = x f32 [S][n], log expression already (must be finite: POLEE_ERR_NONFINITE).  The bias of the reference's embedding stays at
 * zero: the loss sees z through differences only, its exact gradient is zero.
 *   delta_ab = sum_j (lx_aj - lx_bj)^2 / n - (mean_a - mean_b)^2 (pairwise_vlr, :17-26); use_vlr = 0: sum_j (lx_aj - lx_bj)^2 (:42-48)
 *   on a batch I of B sample indices, in order (tsne_p, :136-174): E_ab = clip(exp(-delta_ab / (2 sigma_b^2)), 1e-12, 1), E_aa = 0,
 *     P = (E_ab / sum_a E_ab + E_ba / sum_b E_ba) / (2 S) + eps
 *   on ALL samples (tsne_q, :177-185): k_ij = (1 + |z_i - z_j|^2 / alpha)^(-(alpha + 1) / 2), k_ii = 0, Q = k / sum k, gathered to
 *     I x I, + eps
 *   loss = sum_{a,b in I} P_ab log(P_ab / Q_ab) (:337); samples outside the batch get a gradient through sum k.
 * The draws never leave the device; every sum has a fixed order (no float atomics): every result is bitwise reproducible.
 * Draw rule: the draw with index i uses seed + 0x9E3779B97F4A7C15 i.  polee_tsne_fit: i = t - 1 for Adam step t of the handle's step
 * clock, which runs on across calls, so fit(2) then fit(3) equals fit(5); polee_tsne_distances and polee_tsne_eval: i = 0;
 * polee_tsne_embed: i = its own draw number.
 * POLEE_ERR_BAD_ARG: a batch index outside 0 .. S-1 or repeated within a batch, B < 2 or B > S, bandwidths not set or not positive,
 * an `ap` of another context, n or S. */
typedef struct polee_tsne polee_tsne;
typedef struct {
    int32_t num_components; /* C, --num-components, 2 (tsne.jl:23-27) */
    int32_t use_vlr;        /* 1 (tsne.jl:94) */
    float alpha;            /* 1 (polee_tsne.py:218) */
    float eps;              /* 1e-6, added to P and to Q (:309, :319, :327) */
    float learning_rate;    /* 1e-6 (:344) */
    float beta1, beta2, epsilon; /* tf.train.AdamOptimizer: 0.99, 0.999 (:344-345), 1e-8 */
} polee_tsne_opts;
void polee_tsne_default_opts(polee_tsne_opts *opts);
/* 1 <= num_components <= 16, anything else POLEE_ERR_UNSUPPORTED; opts NULL = the defaults (estimate_tsne, :213-218) */
polee_status polee_tsne_create(polee_ctx *ctx, int32_t n, int32_t S, const polee_tsne_opts *opts, polee_tsne **out);
void polee_tsne_destroy(polee_tsne *ts);
/* W f32 [n][C] (:293-296); set leaves the Adam moments and the step clock alone */
polee_status polee_tsne_get_params(polee_tsne *ts, float *w);
polee_status polee_tsne_set_params(polee_tsne *ts, const float *w);
/* Adam moments and step clock back to zero (a fresh optimiser, :344-347) */
polee_status polee_tsne_reset(polee_tsne *ts);
/* the bandwidths of find_sigmas (:64-103, :238), f32 [S], positive and finite */
polee_status polee_tsne_set_sigmas(polee_tsne *ts, const float *sigmas);
/* delta f64 [S][S] of one draw (what find_sigmas works on, :238); exactly symmetric, diagonal exactly 0; z0_or_null f32 [S][n-1] */
polee_status polee_tsne_distances(polee_tsne *ts, polee_approx *ap, const float *z0_or_null, uint64_t seed, double *delta);
polee_status polee_tsne_distances_points(polee_tsne *ts, const float *x, double *delta);
/* the loss (:337) of one evaluation on the batch i32 [B] and its gradient g_w f32 [n][C] (may be NULL), no update: exactly the
 * numbers a fit step feeds to Adam (the same kernels in the same order) */
polee_status polee_tsne_eval(polee_tsne *ts, polee_approx *ap, const int32_t *batch, int32_t B, const float *z0_or_null, uint64_t seed,
                             float *loss, float *g_w);
polee_status polee_tsne_eval_points(polee_tsne *ts, const float *x, const int32_t *batch, int32_t B, float *loss, float *g_w);
/* niter Adam steps (:355-390), step `it` on the batch batches[it] (i32 [niter][B]): lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t),
 * p -= lr_t m / (sqrt(v) + epsilon).  z0_or_null f32 [niter][S][n-1], uploaded once; loss_trace_or_null f32 [niter].  Nothing waits
 * for the device until the last step is queued.  A call that fails partway keeps the updates of the steps it completed and advances
 * the clock by those. */
polee_status polee_tsne_fit(polee_tsne *ts, polee_approx *ap, const int32_t *batches, int32_t B, int32_t niter, uint64_t seed,
                            const float *z0_or_null, float *loss_trace_or_null);
polee_status polee_tsne_fit_points(polee_tsne *ts, const float *x, const int32_t *batches, int32_t B, int32_t niter,
                                   float *loss_trace_or_null);
/* the mean over ndraws draws of z = lx W (:392-395), accumulated in f64; z0_or_null f32 [ndraws][S][n-1]; z f32 [S][C] */
polee_status polee_tsne_embed(polee_tsne *ts, polee_approx *ap, int32_t ndraws, uint64_t seed, const float *z0_or_null, float *z);
polee_status polee_tsne_embed_points(polee_tsne *ts, const float *x, float *z);

/* ---- `polee model random-forest` (models/random-forest.jl; csrc/forest.hip, csrc/forest_host.cpp, csrc/forest_common.hpp; DESIGN.md
 * section 3.14): a classification forest on log expression, grown level by level for all trees at once on the device.  The forest is
 * this project's own exact definition (integers, Philox counters and correctly rounded f64 additions only): the device builder, the
 * host builder below and the NumPy restatement of the tests give the same node arrays bit for bit.
 * x f32 [N][n] is log expression already and must be finite (POLEE_ERR_NONFINITE); labels are class numbers in 0 .. k-1.
 * A forest is ntrees trees in CSR form: tree t owns the nodes tree_off[t] .. tree_off[t+1]-1 of the five node arrays, numbered level
 * by level from its root 0; left / right are node numbers within the tree (-1 in a leaf), feature is -1 in a leaf, label is the
 * majority class of the node's rows (smallest class on a tie) in every node, threshold is 0 in a leaf.  A row goes left iff
 * (double)x[feature] < threshold.
 * A tree's bootstrap sample has N_b = max(1, floor(partial_sampling N)) rows; N_b > POLEE_FOREST_MAX_ROWS: POLEE_ERR_UNSUPPORTED. */
#define POLEE_FOREST_MAX_ROWS 8192
typedef struct polee_forest polee_forest;
typedef struct {
    int32_t ntrees;            /* 200 (random-forest.jl:40-43) */
    int32_t max_depth;         /* -1: no limit */
    int32_t min_samples_leaf;  /* 1 */
    int32_t min_samples_split; /* 2 */
    double nsubfeatures;       /* 10: nsub = max(1, min(n, round-half-even(nsubfeatures sqrt(n)))) (:44-47, :262) */
    double partial_sampling;   /* 1 (:48-51) */
} polee_forest_opts;
void polee_forest_default_opts(polee_forest_opts *opts);
/* 2 <= k <= 16, anything else POLEE_ERR_UNSUPPORTED; opts NULL = the defaults */
polee_status polee_forest_create(polee_ctx *ctx, int32_t n, int32_t k, const polee_forest_opts *opts, polee_forest **out);
void polee_forest_destroy(polee_forest *f);
polee_status polee_forest_fit_points(polee_forest *f, const float *x, const int32_t *labels, int32_t N, uint64_t seed);
/* Training rows are the logs of ndraws draws of every sample of `ap`: row d S + s is draw d of sample s (draw d uses draw_seed +
 * 0x9E3779B97F4A7C15 d; z0_or_null f32 [ndraws][S][n-1]) and carries labels[s]; `seed` keys the forest. */
polee_status polee_forest_fit(polee_forest *f, polee_approx *ap, const int32_t *labels, int32_t ndraws, uint64_t draw_seed,
                              uint64_t seed, const float *z0_or_null);
polee_status polee_forest_node_count(polee_forest *f, int32_t *ntrees, int64_t *nnodes);
/* tree_off i64 [ntrees+1]; the node arrays [nnodes] */
polee_status polee_forest_get_nodes(polee_forest *f, int64_t *tree_off, int32_t *feature, double *threshold, int32_t *left,
                                    int32_t *right, int32_t *label);
/* Loads a forest built elsewhere (the host builder, a hand-made one).  Checked: every child lies in its tree and after its parent,
 * features in -1 .. n-1, labels in 0 .. k-1, a node has two children or none (else POLEE_ERR_BAD_ARG). */
polee_status polee_forest_set_nodes(polee_forest *f, int32_t ntrees, const int64_t *tree_off, const int32_t *feature,
                                    const double *threshold, const int32_t *left, const int32_t *right, const int32_t *label);
/* votes i32 [R][k]: how many trees sent row r to a leaf of class c */
polee_status polee_forest_predict_points(polee_forest *f, const float *x, int32_t R, int32_t *votes);
/* votes i32 [S][k] summed over the ndraws draws of every sample (draw rule as polee_forest_fit) */
polee_status polee_forest_predict(polee_forest *f, polee_approx *ap, int32_t ndraws, uint64_t seed, const float *z0_or_null,
                                  int32_t *votes);
/* out f32 [ndraws S][n]: the very rows polee_forest_fit trains on and polee_forest_predict walks (the device's log of the draws: taken in f64, rounded to f32 once) */
polee_status polee_forest_log_draws(polee_approx *ap, int32_t ndraws, uint64_t seed, const float *z0_or_null, float *out);
/* The same forest on the host, trees in parallel over POLEE_HOST_THREADS; no context.  With the node arrays NULL it only counts
 * (*nnodes); otherwise it fills them, and POLEE_ERR_BAD_ARG if the forest needs more than `capacity` nodes (ntrees (2 N_b - 1) always
 * suffices).  tree_off i64 [ntrees+1]. */
polee_status polee_forest_build_host(const float *x, const int32_t *labels, int32_t N, int32_t n, int32_t k,
                                     const polee_forest_opts *opts, uint64_t seed, int64_t capacity, int64_t *nnodes,
                                     int64_t *tree_off, int32_t *feature, double *threshold, int32_t *left, int32_t *right,
                                     int32_t *label);
polee_status polee_forest_votes_host(int32_t n, int32_t k, int32_t ntrees, const int64_t *tree_off, const int32_t *feature,
                                     const double *threshold, const int32_t *left, const int32_t *right, const int32_t *label,
                                     const float *x, int32_t R, int32_t *votes);

/* ---- training of the fragment bias model (src/bias.jl; csrc/bias_train.hip, csrc/bias_train_host.cpp, csrc/bias_train_common.hpp;
 * DESIGN.md section 3.16): from training fragments to the tables polee_xb_biasmodel takes.  The two sequence models by the greedy BIC
 * search over variable-order Markov chains (SeqBiasModel, bias.jl:266-399), the GC histogram (SimpleHistogramModel, bias.jl:464-514) and
 * the accuracy figure (bias.jl:788-828).  Not here: PositionalBiasModel (use_pos_bias = false in every caller of the reference), and the
 * steps BEFORE the training fragments -- subsampling reads, the SimplisticFragModel's estimation, the EM assignment of each read to one
 * transcript and its projection to (tpos, fraglen) (rnaseq_sample.jl:330-377, fragmodel.jl:205-246) -- which stay upstream.
 * The model is this project's own exact definition where the reference is not reproducible: positions beyond a transcript's ends are
 * Philox nucleotides (randdna in the reference, bias.jl:83-101), a drawn background position is a Philox draw (rand, fragmodel.jl:243),
 * and the log of the loss is taken and summed in f64 in a fixed order (Float32 log and pairwise sum in bias.jl:254-257).  The device
 * trainer, the host trainer (host = 1; POLEE_HOST_THREADS) and the NumPy restatement of the tests give the same model bit for bit; the
 * loss trace agrees to the ulp error of log.
 * 30 <= n_fg + n_bg (POLEE_ERR_BAD_ARG below: the reference leaves quantiles uninitialised) < 2^24 (POLEE_ERR_UNSUPPORTED from there:
 * counts are exact f32 integers below). */
typedef struct polee_bias_train polee_bias_train;
typedef struct {
    uint64_t seed;    /* keys the pads and the drawn background */
    int32_t host;     /* 1: the host trainer; ctx may then be NULL */
    int32_t reserved; /* 0 */
} polee_bias_train_opts;
/* Examples from fragments (BiasTrainingExample, bias.jl:21-80; extract_padded_seq, :88-102).  tseq_ptr [n+1] / tseq as in
 * polee_xb_biasmodel.  Fragments are (transcript 0-based, tpos 1-based in transcript orientation, fraglen); required of each:
 * fraglen >= 20, tpos >= 1, tpos + fraglen - 1 <= tlen (fragmodel.jl:227-234), else POLEE_ERR_BAD_ARG.  bg_transcript NULL: one
 * background fragment per foreground fragment is drawn, same transcript and length, tpos uniform in 1 .. tlen - fraglen + 1
 * (fragmodel.jl:243); n_bg, bg_tpos and bg_fraglen are then ignored.  opts NULL: seed 0, on the device. */
polee_status polee_bias_train_create(polee_ctx *ctx, int32_t n, const int64_t *tseq_ptr, const uint8_t *tseq, int64_t n_fg,
                                     const int32_t *fg_transcript, const int64_t *fg_tpos, const int32_t *fg_fraglen, int64_t n_bg,
                                     const int32_t *bg_transcript, const int64_t *bg_tpos, const int32_t *bg_fraglen,
                                     const polee_bias_train_opts *opts, polee_bias_train **out);
/* Ready-made examples (the reference's --dump-bias-training-examples files, fragmodel.jl:306-339): left_seq / right_seq u8 [N][20]
 * codes (0 A, 1 C, 2 G, 3 T, other -> A: nt2bit, bias.jl:176-181), frag_gc f64 [N] in 0 .. 1; N = n_fg + n_bg, foreground first. */
polee_status polee_bias_train_create_from_examples(polee_ctx *ctx, int64_t n_fg, int64_t n_bg, const uint8_t *left_seq,
                                                   const uint8_t *right_seq, const double *frag_gc, const polee_bias_train_opts *opts,
                                                   polee_bias_train **out);
void polee_bias_train_destroy(polee_bias_train *bt);
/* BiasModel(...) (bias.jl:677-785): both sequence models, the GC model, the accuracy */
polee_status polee_bias_train_run(polee_bias_train *bt);
/* The trained model in polee_xb_biasmodel's layout (each pointer may be NULL): orders i32 [20]; ps f32 [20][4][4096] = ps_fg / ps_bg
 * (bias.jl:398), 1.0 where the model never reads (order -1, contexts >= 4^order; NaN in the reference); gc_bins f32 [100] (bias.jl:505-511)
 * and the 14 quantile boundaries behind them, gc_qs (bias.jl:476-489); accuracy (bias.jl:788-828) as a fraction. */
polee_status polee_bias_train_get_model(polee_bias_train *bt, int32_t *orders_left, int32_t *orders_right, float *ps_left, float *ps_right,
                                        float *gc_bins, float *gc_qs, double *accuracy);
/* The examples as the trainer holds them (each pointer may be NULL): left / right u64 [N], 20 two-bit codes each, position 1 in bits
 * 39:38 (bias.jl:283-293); frag_gc f64 [N] (bias.jl:63); bg_tpos i64 [n_bg], the background positions given or drawn
 * (fragmodel.jl:243; POLEE_ERR_BAD_ARG for a trainer made from examples). */
polee_status polee_bias_train_get_examples(polee_bias_train *bt, int64_t *n_fg, int64_t *n_bg, uint64_t *left, uint64_t *right,
                                           double *frag_gc, int64_t *bg_tpos);
/* The search of one side (0 left, 1 right; bias.jl:353-396): *rounds committed rounds (<= 140), positions i32 [rounds] (0-based, the
 * position whose order each round raised), losses f64 [rounds + 1] (loss0 at the start, bias.jl:352, and after every round, :393). */
polee_status polee_bias_train_get_trace(polee_bias_train *bt, int32_t side, int32_t *rounds, int32_t *positions, double *losses);
/* Debug entry: scores ONE round (bias.jl:357-383) from a caller-given state.  orders_in i32 [20] (-1 .. 6, position j (1-based) + order
 * <= 20); the tables and factor columns of that state are rebuilt, n_params = sum of 4^(1 + order) over the included positions;
 * losses_out f64 [20] (+inf where no candidate is allowed, bias.jl:358), *loss0_out the loss of the state itself (bias.jl:243-263).
 * Leaves a trained model untouched. */
polee_status polee_bias_train_candidates(polee_bias_train *bt, int32_t side, const int32_t *orders_in, double *losses_out,
                                         double *loss0_out);

/* ---- Splicing features from the transcripts' exon structure (splice_features.hip, host twin splice_features_host.cpp):
 * splicing_features (src/splicing.jl:98-230) over get_introns, get_cassette_exons, get_alt_donor_acceptor_sites and get_alt_fp_tp_ends
 * (src/transcripts.jl:545-950), restated as written.  transcripts: as polee_xbuild_run takes them, every transcript with at least one
 * exon, exons ascending and disjoint; transcript ids in the result are 1-based positions.  gene_of_or_null: i32 [n], the 1-based gene of
 * every transcript; with it the alternative 5' / 3' ends are made too (alt_ends = true), without it they are left out.
 * COORDINATE RANGE: 1 <= first <= last <= 2^31 - 2 (keys carry first - 1 and last + 1 in 32 bits); anything outside, fewer than one
 * exon, a negative sequence id, a strand outside -1 .. +1 or a gene number below 1 is refused with POLEE_ERR_BAD_ARG.
 * The result, F features in the blocks cassette_exon, mutex_exon, alt_acceptor_site / alt_donor_site (one block), retained_intron, alt_5p_end,
 * alt_3p_end; within a block ascending by (seq, strand, included_first, included_last, excluded_first, excluded_last) -- mutex exons with
 * equal unions by their outer interval -- and the alternative ends by (gene, start clusters before end clusters, cluster start): the project's
 * own order (upstream's is that of its interval collections and Dicts).
 *   type i32 [F]       0 cassette_exon, 1 mutex_exon, 2 alt_acceptor_site, 3 alt_donor_site, 4 retained_intron, 5 alt_5p_end, 6 alt_3p_end
 *   seq i32 [F], strand i8 [F]; coords i64 [F][4] = included_first, included_last, excluded_first, excluded_last (-1 where the
 *   reference's table holds -1); end_span i64 [F][2] = (min_first, max_last) of an alternative end's gene as upstream computes them
 *   (max_last is the MINIMUM of the ends, transcripts.jl:884), -1 elsewhere
 *   included_ptr / excluded_ptr i64 [F+1], 0-based into included_idx / excluded_idx i32: the transcripts, ascending and unique
 * polee_splice_run works on the device and is the same from run to run; polee_splice_run_host builds the same arrays element for
 * element on POLEE_HOST_THREADS without a GPU.  POLEE_ERR_UNSUPPORTED from the device path when the member rows before repeats are
 * dropped number 2^32 or more.  POLEE_BUILD_TIMING=1: the phases on stderr. */
typedef struct polee_splice polee_splice;
polee_status polee_splice_run(polee_ctx *ctx, const polee_xb_transcripts *transcripts, const int32_t *gene_of_or_null, polee_splice **out);
polee_status polee_splice_run_host(const polee_xb_transcripts *transcripts, const int32_t *gene_of_or_null, polee_splice **out);
void polee_splice_destroy(polee_splice *sf);
/* each pointer may be NULL; num_overlapping_pairs: unordered pairs of overlapping internal exons of one sequence and strand */
polee_status polee_splice_sizes(const polee_splice *sf, int64_t *num_features, int64_t *num_included, int64_t *num_excluded, int64_t *num_exons,
                                int64_t *num_internal_exons, int64_t *num_overlapping_pairs);
/* copies the result to host arrays (any pointer may be NULL) */
polee_status polee_splice_get(const polee_splice *sf, int32_t *type, int32_t *seq, int8_t *strand, int64_t *coords, int64_t *end_span,
                              int64_t *included_ptr, int32_t *included_idx, int64_t *excluded_ptr, int32_t *excluded_idx);

#ifdef __cplusplus
}
#endif
#endif /* POLEE_HIP_H */
