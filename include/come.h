/*
 * come.h -- C-ABI of the MI355X-native ComE hot path (libcome.so, gfx950).
 *
 * Drop-in boundary for the reference's Cython kernel module
 * (`from utils.training_sdg_inner import train_o1, train_o2, FAST_VERSION`,
 *  /root/reference/ADSCModel/node_embeddings.py:13, context_embeddings.py:14) and for the numpy /
 * sklearn hot loops of /root/reference/ADSCModel/community_embeddings.py.
 *
 * Conventions
 *  - Every pointer named "device" is a non-owning device pointer (the caller owns the buffer, e.g.
 *    a torch tensor); tables are C-contiguous row-major fp32 [rows x d], exactly the layout the
 *    reference's numpy arrays have (pyx:410-411,457-459).
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *    asynchronous on that stream, capture-safe (no allocation / synchronisation inside) once
 *    come_init() has run for the device, and reentrant per stream.  Launch options: each call
 *    reads ONE consistent snapshot of the process-wide options (come_set_option, mutex-guarded:
 *    a change applies to calls that start after it returns, never half of one); the *_ex entry
 *    points take per-call options instead (come_launch_opts), so concurrent callers with
 *    different options do not interfere.
 *  - Return value: 0 = ok, < 0 = error (COME_E_*); come_last_error() returns a message
 *    (thread-local).  The reference checks nothing (bounds checks off, cython_utils.py:7); this
 *    library validates shapes/arguments on the host and never reads or writes out of bounds on
 *    the device: walk entries outside [0, V) are treated as None (pyx:435-436), table draws
 *    outside [0, V) are skipped.
 *  - Row index = the reference's Vocab.index (rank of the node id, model.py:60-64).
 */
#ifndef COME_H_
#define COME_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 5 (no signature or struct changed): the launch option "walk_staged" accepts 0 / 1 only; the
 * A/B values 2 / 3 (8- and 32-step slices of the same walks) are COME_E_INVALID at come_random_walks.
 * ABI 5, additive: come_edge_cdf, come_edge_sample, their CPU twins come_cpu_edge_cdf,
 * come_cpu_edge_sample and the test-support entry come_cpu_edge_pick (edges sampled by weight for
 * the O1 trainer; come_sgns_o1 is unchanged).
 * ABI 5, additive: come_topk_scratch, come_row_sqnorms, come_topk and the CPU twin come_cpu_topk
 * (exact top-k neighbour search over an embedding table).
 * ABI 5, additive: come_walk_cdf, come_random_walks_w and their CPU twins come_cpu_walk_cdf,
 * come_cpu_random_walks_w (edge-weighted walks; the unweighted walkers are unchanged).
 * ABI 5, additive: come_random_walks_pq and its CPU twin come_cpu_random_walks_pq (node2vec
 * (p, q) second-order walks; come_random_walks is unchanged).
 * ABI 5, additive: come_gmm_estep_diag, come_gmm_diag_scratch, come_gmm_diag_moments,
 * come_gmm_diag_scatter, come_community_grad_diag and come_community_loss_diag (diagonal
 * covariances: the GMM EM, the community step and the community loss for covariance_type='diag').
 * ABI 5, additive: come_sgns_o2_loss, come_sgns_pairs_loss and their CPU twins (the SGNS
 * objectives O2 / O1 evaluated natively; read-only on the tables).
 * ABI 5, additive: come_kmeans_pp_scratch, come_kmeans_pp_step, come_kmeans_pp_pick and
 * come_kmeans_pp_sample (the greedy k-means++ seeding of come_amd.kmeans).
 * ABI 5, additive (the version is unchanged: nothing that existed moved): come_kmeans_scratch,
 * come_kmeans_lloyd, come_kmeans_assign and come_kmeans_update (k-means for the GMM init and
 * come_amd.kmeans.KMeans).
 * ABI 5 (this header): "gmm_cov_async" accepts 3 / 4 / 5.  Its default 4 now runs k_gmm_cov_fb3 at
 * d = 128 (the staging inside the MFMA wavefronts; the diagonal 32x32 tiles' cross terms taken as
 * U + U^T, so their fp32 rounding differs from ABI 4's at the same fp32-level error; off-diagonal
 * tiles are bit-identical) and k_gmm_cov_bf3 at d = 64; 5 runs ABI 4's k_gmm_cov_bf3 at both widths.
 * ABI 4: the launch options "community_async" accept 2 / 3, "gmm_cov_async" 3 / 4
 * and "gmm_resp16" 2 / 3 only -- the 32x32 fp32 fallbacks that ABI 3's values 1 / 1 / 0 selected
 * were removed (COME_E_INVALID at the call now) -- and their defaults became the bf16-part MFMA
 * kernels (3 / 4 / 3: fp32 operands as three bf16 parts, fp32-level error).
 * ABI 3: the launch option "gmm_resp_db" (the double-buffered 32x32 E-step A/B kernels) was
 * removed, "community_async" accepts 1 / 2 / 3, "gmm_cov_async" 1 / 3 / 4 and "gmm_resp16"
 * 0 / 2 / 3 (other values: COME_E_INVALID at the call); come_source_sha256 was added.
 * ABI 2: come_*_ex hot_rows == NULL in COME_MODE_HOGWILD now means "derive the
 * contended-row bitmap from the table" (ABI 1: every row cold; now COME_HOT_NONE); the launch
 * options "o2_plain_writeback" and "o2_pair_atomics" (ABI 1, ring-kernel Hogwild) were removed and
 * come_set_option rejects them; o2_kernel = 2 with COME_MODE_HOGWILD returns COME_E_INVALID. */
#define COME_ABI_VERSION 5

enum {
    COME_OK = 0,
    COME_E_INVALID = -1, /* bad argument (message in come_last_error) */
    COME_E_HIP = -2,     /* HIP runtime error */
    COME_E_UNSUPPORTED = -3
};

enum {
    COME_MODE_HOGWILD = 0,    /* one wavefront per walk/edge, all walks/edges in flight (the
                                 reference's per-walk Hogwild threads, pyx:493) */
    COME_MODE_SEQUENTIAL = 1  /* one wavefront, walks/edges in order == workers=1: the parity
                                 anchor, bit-exact with oracle/ in its WAVE64 dot order */
};

/* Flag OR-ed into `mode` of come_sgns_o2 / come_sgns_o1: `table` points to come_pack_table's
 * packed words (T still the logical number of slots) instead of the uint32 table. */
#define COME_TABLE_PACKED 0x100

/* Flag OR-ed into `mode` (COME_MODE_HOGWILD): no contended rows -- every row is updated with plain
 * stores, hot_rows ignored.  Without it a NULL hot_rows makes the library derive the bitmap. */
#define COME_HOT_NONE 0x200

/* Share of the negative table from which a row counts as contended when the library derives the
 * bitmap itself: rows holding >= max(1, floor(share * T)) slots, share = COME_DEFAULT_HOT_SHARE
 * for rows of d <= 128 and COME_DEFAULT_HOT_SHARE_WIDE for wider rows
 * (come_amd.training_sdg_inner.default_hot_share; measured in DESIGN.md §3.1: with d = 256 and
 * 10 negatives, plain stores on rows between the two shares lose enough concurrent updates on a
 * 1M-node power-law graph to move the held-out loss 1.8% below the reference's). */
#define COME_DEFAULT_HOT_SHARE 5e-6
#define COME_DEFAULT_HOT_SHARE_WIDE 8e-7

int come_abi_version(void);

/* SHA-256 (hex) of the sources the library was built from (the csrc .hip / .cpp / .h files, the Makefile
 * and this header, concatenated in name order): the Python binding refuses a library whose stamp
 * differs from the sources beside it. */
const char *come_source_sha256(void);
const char *come_last_error(void);

/* Uploads the sigmoid table (pyx:531-533) to `device`'s constant memory.  Called implicitly by the
 * first launch on a device; call it explicitly before capturing a stream into a hipGraph. */
int come_init(int device);

/* Host: the reference's EXP_TABLE (pyx:92-95,531-533), 1000 floats. Replaces the module-global
 * table built by init() (pyx:512). */
void come_exp_table(float *out1000);

/* Host: value of the reference's FAST_VERSION (pyx:549).  Always 0: the dot product is consumed
 * as float after a double-width reduction, like fast0_* (pyx:140). */
int come_fast_version(void);

/* ---- SGNS, second order (context over walks): replaces train_o2 (pyx:454-509) over a batch ----
 * node, ctx   device fp32 [V x d] (node_embedding / context_embedding), updated in place.
 * walks       device int32 [P x L] row indices; -1 (or any value outside [0,V)) = None; trailing
 *             padding with -1 is equivalent to a shorter walk.  L <= 10000 (MAX_SENTENCE_LEN,
 *             pyx:18,480).
 * seeds       device uint64 [P], walk p's initial next_random (pyx:477: 2^24*randint+randint).
 * table       device uint32 [T] negative-sampling table (model.py:97-122), values are rows.
 * negative    0..20;  window >= 0;  1 <= d <= 512.
 * The number of pair updates a batch performs is come_count_o2_pairs() of its walks.
 * COME_MODE_HOGWILD: the contended rows are derived from `table` per call (as come_sgns_o2_ex with
 * hot_rows == NULL); OR COME_HOT_NONE into `mode` to treat every row as cold.
 */
int come_sgns_o2(float *node, float *ctx, int64_t V, int d, const int32_t *walks, int64_t P,
                 int L, const uint64_t *seeds, int window, int negative, const uint32_t *table,
                 uint64_t T, float lr, float alpha, int mode, void *stream);

/* ---- Packed negative table: an exact, 16x smaller equivalent of make_table's output ----
 * packed: device, 16 * ceil(T / 64) bytes, 16-byte aligned; word w = {uint32 base = table[64w],
 * uint32 0, uint64 bits} with bit i (1..63) set iff table[64w+i] == table[64w+i-1] + 1, so
 * table[64w+i] = base + popcount(bits & (2^(i+1) - 1)).  Exact when every step inside a word is
 * 0 or 1, which make_table guarantees (model.py:107-121 advances at most one id per slot).
 * status: device int32, set to 0 if the table packed exactly, 1 if some step was not 0/1 (then
 * the packed words must not be used).  Asynchronous on `stream`. */
int come_pack_table(const uint32_t *table, uint64_t T, void *packed, int32_t *status,
                    void *stream);

/* ---- SGNS, first order (edges): replaces train_o1 (pyx:407-450) over a batch ----
 * edges       device int32 [E x 2] rows (u, v): pair (input u, positive v) then (input v,
 *             positive u), RNG state carried across both (pyx:444-448).
 * seeds       device uint64 [E], edge e's initial next_random (pyx:427). */
int come_sgns_o1(float *node, int64_t V, int d, const int32_t *edges, int64_t E,
                 const uint64_t *seeds, int negative, const uint32_t *table, uint64_t T, float lr,
                 int mode, void *stream);

/* ---- SGNS losses: the objective of a come_sgns_o2 batch, and of explicit pair lists ----
 * For an input row a of table `inp`, a positive row b and negative rows t_1..t_n of table `out`:
 *   pair(a; b; t) = softplus(-f(a, b)) + sum_k softplus(f(a, t_k)),   softplus(z) = log(1 + e^z)
 * i.e. -log s(a.b) - sum_k log s(-a.t_k), the exact objective: neither the trainer's +-6 skip nor
 * its 1000-entry sigmoid table.  f is the trainer's own fp32 dot (element e in lane e % 64, slot
 * e / 64, an fmaf chain per lane in slot order, the lanes summed by the xor butterfly over offsets
 * 1..32); softplus is evaluated in float64 on that fp32 value as max(z, 0) + log1p(exp(-|z|)).
 * Summation order is part of the contract: a pair's terms are added in k order (k = 0 the
 * positive) in float64, a walk's pairs in the trainer's pair order, and a total is the sum of the
 * per-walk (per-pair) values in index order by a fixed tree (blocks of 4096 values: thread t of
 * 256 adds values t, t + 256, ... then a halving tree; the block sums the same way).  No float or
 * double atomics: every output is bit-identical from run to run, and the total does not depend on
 * whether the per-walk / per-pair output is requested.  Both calls only read the tables, are
 * asynchronous on `stream` and use library scratch that grows on demand (the first call at a
 * larger P / M allocates: warm up before capturing a stream, as for come_sgns_o2_ex's bitmap).
 * Tables, walks and row lists need only their natural 4-byte alignment.  P and M must be below
 * 2^31 (COME_E_INVALID above; the CPU twins hold the same limit).
 *
 * come_sgns_o2_loss: the objective of exactly the batch come_sgns_o2 would train on with these
 * walks and seeds.  Pairs as pyx:494-508 (centre i gives the positive row in ctx, every valid j of
 * its window the input row in node, i outer, j inner; walk entries outside [0, V) are None); the
 * `negative` draws of a pair are table[(next_random >> 16) % T] followed by the LCG step
 * (pyx:133-134), next_random starting at seeds[p] and carried through the walk.  Every draw
 * advances the LCG; a draw equal to the positive row (pyx:135) or outside [0, V) is skipped.
 * flags: 0 or COME_TABLE_PACKED.  negative 0..20 (0: table may be NULL); any window >= 0;
 * L <= 10000; 1 <= d <= 512.  walk_out: device float64 [P] or NULL; loss_out: one device double;
 * pairs_out: one device int64 or NULL, = come_count_o2_pairs of the walks.  P = 0 is a no-op
 * returning 0 that writes nothing; P > 0 without a pair writes 0.0 and 0.
 *
 * come_sgns_pairs_loss: explicit lists (held-out evaluation, O1): rows_in, rows_pos device int32
 * [M], rows_neg device int32 [M x negative] row-major (NULL when negative = 0).  A pair whose
 * input or positive row is outside [0, V) contributes 0 and is not counted; a negative outside
 * [0, V) is skipped; a negative equal to the positive is used as given (the caller's list is the
 * truth).  inp may equal out (O1).  pair_out: device float64 [M] or NULL; loss_out / pairs_out as
 * above (pairs_out = the pairs counted).  M = 0 is a no-op returning 0. */
int come_sgns_o2_loss(const float *node, const float *ctx, int64_t V, int d, const int32_t *walks,
                      int64_t P, int L, const uint64_t *seeds, int window, int negative,
                      const uint32_t *table, uint64_t T, int flags, double *walk_out,
                      double *loss_out, int64_t *pairs_out, void *stream);
int come_sgns_pairs_loss(const float *inp, const float *out, int64_t V, int d,
                         const int32_t *rows_in, const int32_t *rows_pos, const int32_t *rows_neg,
                         int64_t M, int negative, double *pair_out, double *loss_out,
                         int64_t *pairs_out, void *stream);

/* ---- Community gradient: replaces Community2Vec.train (community_embeddings.py:61-78) ----
 * x [V x d] updated in place, `iters` times:
 *   x_i -= lr * clip((beta/K) * sum_k pi[i,k] * inv_cov[k] @ (x_i - mu[k]), -5, 5)
 * pi [V x K], mu [K x d], inv_cov [K x d x d] (all device fp32).  1 <= d <= 512 (MFMA kernels at
 * d = 64, 128; VALU forms otherwise, the d x d matrices streamed in row chunks above d = 128). */
int come_community_grad(float *x, int64_t V, int d, const float *pi, const float *mu,
                        const float *inv_cov, int K, float beta, float lr, int iters,
                        void *stream);

/* ---- Community loss: the objective come_community_grad descends, what Community2Vec.loss
 * (community_embeddings.py:40-59) is meant to compute ----
 *   row_i = sum_k pi[i,k] * (log_norm[k] - |x_i prec_chol[k] - mu_prec[k]|^2 / 2),  total = sum_i row_i
 * i.e. sum_k pi[i,k] log N(x_i; mu_k, Sigma_k) when prec_chol[k] is the precision Cholesky factor
 * of Sigma_k, mu_prec[k] = mu_k @ prec_chol[k] and log_norm[k] = log det(prec_chol[k]) - d/2
 * log(2 pi) -- come_gmm_estep's operands with NO mixture weight in log_norm.  x [V x d], pi
 * [V x K] (used as given: rows need not sum to 1), prec_chol [K x d x d], mu_prec [K x d],
 * log_norm [K] (all device fp32); row_out [V] device fp32 or NULL; loss_out one device double
 * (the rows summed in float64).  1 <= d <= 512, 1 <= K <= 4096 for every d.
 * prec_chol MUST hold upper-triangular factors with zeros below the diagonal (what come_gmm_params
 * writes): the kernels for d = 64, 128 never read most of the lower triangle and there is no
 * check and no fallback for a lower or dense factor (unlike come_gmm_estep).  d = 64, 128 with
 * 16-byte aligned x, prec_chol and mu_prec run come_gmm_estep's bf16-part MFMA stream, anything
 * else a VALU kernel.  No float or double atomics: row_out and loss_out are bit-identical from run
 * to run, and loss_out does not depend on whether row_out is given.  V = 0 is a no-op returning 0
 * (loss_out is not written).  Asynchronous on `stream`. */
int come_community_loss(const float *x, int64_t V, int d, const float *pi, const float *prec_chol,
                        const float *mu_prec, const float *log_norm, int K, float *row_out,
                        double *loss_out, void *stream);

/* ---- GMM responsibilities: replaces GaussianMixture.predict_proba (community_embeddings.py:37)
 * for covariance_type='full'.  prec_chol [K x d x d] (precision Cholesky factors, sklearn
 * layout), mu_prec [K x d] = mu_k @ prec_chol_k, log_norm [K] = log w_k + log det(prec_chol_k)
 * - d/2 log(2 pi) (all device fp32, precomputed on the host from the fitted parameters).
 * resp_out [V x K] device fp32.  1 <= d <= 512.  K <= 64 for d <= 128 other than 64 and 128;
 * K <= 4096 for d = 64, 128 and for d > 128 (those kernels keep the per-component
 * log-probabilities in resp_out itself). */
int come_gmm_resp(const float *x, int64_t V, int d, const float *prec_chol, const float *mu_prec,
                  const float *log_norm, int K, float *resp_out, void *stream);

/* ---- GMM EM fit (replaces GaussianMixture.fit, community_embeddings.py:27; sklearn
 * BaseMixture.fit_predict / _e_step / _m_step for covariance_type='full') ----
 * E-step: come_gmm_resp plus lse_out [V] = per-row log sum_k exp(log w_k + log N(x; mu_k, S_k))
 * (the mean of lse_out is sklearn's log_prob_norm / lower bound).  log_norm[k] may be -inf (a
 * component of weight zero): such a component gets responsibility exactly 0 and adds nothing to
 * lse_out, as long as some component of the launch is finite. */
int come_gmm_estep(const float *x, int64_t V, int d, const float *prec_chol, const float *mu_prec,
                   const float *log_norm, int K, float *resp_out, float *lse_out, void *stream);

/* M-step scatter matrices: scatter_out [K x d x d] = sum_i resp[i,k] (x_i - means_k)
 * (x_i - means_k)^T (device fp32; covariance_k = scatter_k / nk_k + reg_covar I, sklearn
 * _estimate_gaussian_covariances_full).  Rows are split into `chunks` partial sums reduced in a
 * fixed order (deterministic); scratch: device fp32 [chunks x K x d x d] (unused when
 * chunks == 1).  1 <= d <= 512. */
int come_gmm_scatter(const float *x, int64_t V, int d, const float *resp, const float *means,
                     int K, int chunks, float *scratch, float *scatter_out, void *stream);

/* The rest of one M-step and the E-step parameters it implies, one workgroup per component, in
 * float64 (sklearn _estimate_gaussian_covariances_full + _compute_precision_cholesky +
 * _estimate_log_gaussian_prob's constants): cov_out [K x d x d] = scatter_k / nk_k + reg_covar I,
 * its Cholesky factor L, prec_chol_out [K x d x d] = L^-T (upper), and the E-step's fp32 inputs:
 * e_prec_chol [K x d x d] = prec_chol, e_mu_prec [K x d] = means_k prec_chol_k, e_log_norm [K] =
 * log weights_k + sum log diag(prec_chol_k) - d/2 log(2 pi).  info [K] (device int32): 0, or j + 1
 * when the j-th pivot of component k's Cholesky factorisation is not positive (sklearn raises;
 * the caller checks).  All pointers are device memory; 1 <= d <= 128. */
int come_gmm_params(const double *scatter, const double *nk, const double *means,
                    const double *weights, int K, int d, double reg_covar, double *cov_out,
                    double *prec_chol_out, float *e_prec_chol, float *e_mu_prec,
                    float *e_log_norm, int *info, void *stream);

/* ---- Diagonal covariances (sklearn covariance_type='diag'): Sigma_k = diag(var_k) ----
 * The same steps as above with d parameters per component instead of d (d + 1) / 2: fp32 VALU
 * streams over one read of x, for every 1 <= d <= 512 and 1 <= K <= 4096 alike.  All tables are
 * device fp32, row-major, and need 4-byte alignment only.  No float or double atomics: every
 * output is bit-identical from run to run.  Asynchronous on `stream`.
 * Component operands: prec_sqrt [K x d] = 1 / sqrt(var) (sklearn's precisions_cholesky_),
 * mu_prec [K x d] = mu * prec_sqrt, log_norm [K] = log w_k + sum_j log prec_sqrt[k][j] - d/2
 * log(2 pi) (without log w_k for the loss); the log-density of (row i, component k) is
 * log_norm[k] - 1/2 sum_j (x[i][j] prec_sqrt[k][j] - mu_prec[k][j])^2.
 *
 * come_gmm_estep_diag: resp_out [V x K] and lse_out [V] as come_gmm_estep defines them; resp_out
 * may be NULL (lse_out only, bitwise the same).  log_norm[k] = -inf: responsibility exactly 0,
 * nothing added to lse_out.  V = 0 is a no-op.
 *
 * come_gmm_diag_scratch (host): the row chunking of the two M-step passes for a device with `cus`
 * compute units (<= 0: 256): chunks_out >= 1 with chunks * (K d + K) * 4 <= 128 MB, the size in
 * bytes of their `scratch` (unused when chunks == 1), and rows_per_chunk_out = ceil(V / chunks),
 * an upper bound on the rows summed in fp32 before the float64 reduction.
 *
 * come_gmm_diag_moments: nk_out [K] = sum_i resp[i][k] and sx_out [K x d] = sum_i resp[i][k]
 * x[i][j] (device float64); per-chunk fp32 partials reduced in chunk order in float64.
 *
 * come_gmm_diag_scatter: ssq_out [K x d] = sum_i resp[i][k] (x[i][j] - means[k][j])^2 (device
 * float64; means [K x d] fp32), centred as come_gmm_scatter is; chunking as the moments.
 *
 * come_community_grad_diag: come_community_grad with inv_cov[k] = diag(inv_var[k]), inv_var
 * [K x d]: x[i][j] -= lr * clip((beta / K) sum_k pi[i][k] inv_var[k][j] (x[i][j] - mu[k][j]),
 * +-5), `iters` times in place.  pi is used as given.
 *
 * come_community_loss_diag: come_community_loss's contract (row_out [V] or NULL, loss_out one
 * device double, the total independent of row_out, V = 0 a no-op that leaves loss_out unwritten). */
int come_gmm_estep_diag(const float *x, int64_t V, int d, const float *prec_sqrt,
                        const float *mu_prec, const float *log_norm, int K, float *resp_out,
                        float *lse_out, void *stream);
int come_gmm_diag_scratch(int64_t V, int d, int K, int cus, int *chunks_out,
                          int *rows_per_chunk_out);
int come_gmm_diag_moments(const float *x, int64_t V, int d, const float *resp, int K, int chunks,
                          void *scratch, double *nk_out, double *sx_out, void *stream);
int come_gmm_diag_scatter(const float *x, int64_t V, int d, const float *resp, const float *means,
                          int K, int chunks, void *scratch, double *ssq_out, void *stream);
int come_community_grad_diag(float *x, int64_t V, int d, const float *pi, const float *mu,
                             const float *inv_var, int K, float beta, float lr, int iters,
                             void *stream);
int come_community_loss_diag(const float *x, int64_t V, int d, const float *pi,
                             const float *prec_sqrt, const float *mu_prec, const float *log_norm,
                             int K, float *row_out, double *loss_out, void *stream);

/* ---- k-means (Lloyd): the GMM's initialisation (sklearn KMeans inside GaussianMixture, reference
 * community_embeddings.py:27) and come_amd.kmeans.KMeans ----
 * x [V x d] rows, centers [K x d] (device fp32).  1 <= d <= 512; 1 <= K <= 64, K <= 4096 for
 * d = 64, 128 and d > 128 (GaussianMixture's limits).  A row's label is the argmax over k of
 * s_k = x . c_k - |c_k|^2 / 2 (= the argmin of the squared distance), ties to the lowest k;
 * mindist = max(0, |x|^2 - 2 s_label).  d = 64, 128 with K <= 64 and 16-byte aligned x and
 * centers run on fp32 MFMAs (scores, and the cluster sums as a one-hot x X product), anything else
 * on a VALU kernel.  No float atomics: every output is bit-identical from run to run.
 *
 * come_kmeans_scratch (host): the row chunking of come_kmeans_lloyd for a device with `cus` compute
 * units (<= 0: 256): chunks_out >= 1 with chunks * K * d * 4 <= 128 MB, and rows_per_chunk_out, an
 * upper bound on the rows whose cluster sums are accumulated in fp32 before the float64 reduction
 * (a multiple of 16).  V must be >= 1.  The scratch of come_kmeans_lloyd is
 * chunks * (8 + 4 K d + 4 K) bytes, 8-byte aligned.
 *
 * come_kmeans_lloyd: one pass over x: labels_out [V] (int32), mindist_out [V] (optional), and the
 * per-chunk partial sums / counts / inertia into `scratch`, reduced in chunk order into sums_out
 * [K x d] (float64: sum of the rows of each cluster), counts_out [K] (int64) and inertia_out
 * (float64: the sum of mindist, accumulated in float64).  V must be >= 1 (an empty pass would
 * still have to write its outputs).
 *
 * come_kmeans_assign: labels_out and (optionally) mindist_out only, by the same arithmetic.
 * V = 0 is a no-op returning 0.
 *
 * come_kmeans_update: centers_k = (float)(sums_k / counts_k) in place; a cluster with count 0 keeps
 * its centre bit for bit.  stats2[0] = sum (new - old)^2 in float64 (stats2[1] is not written).
 * Reduction and update are separate so that a distributed fit can all-reduce sums and counts
 * between them. */
int come_kmeans_scratch(int64_t V, int d, int K, int cus, int *chunks_out,
                        int *rows_per_chunk_out);
int come_kmeans_lloyd(const float *x, int64_t V, int d, const float *centers, int K, int chunks,
                      void *scratch, int32_t *labels_out, float *mindist_out, double *sums_out,
                      int64_t *counts_out, double *inertia_out, void *stream);
int come_kmeans_assign(const float *x, int64_t V, int d, const float *centers, int K,
                       int32_t *labels_out, float *mindist_out, void *stream);
int come_kmeans_update(float *centers, const double *sums, const int64_t *counts, int K, int d,
                       double *stats2, void *stream);

/* ---- greedy k-means++ seeding (sklearn's _kmeans_plusplus with T local trials per step) ----
 * One step: come_kmeans_pp_step on the T candidates, come_kmeans_pp_pick, come_kmeans_pp_sample
 * for the next step's candidates.  Nothing is read by the host: the candidates, the choice and the
 * potentials stay on the device.  x [V x d] device fp32, not necessarily 16-byte aligned;
 * 1 <= V < 2^31, 1 <= d <= 512, 1 <= T <= 16.  No float atomics: every output is bit-identical
 * from run to run.
 *
 * come_kmeans_pp_scratch (host): the row chunking for a device with `cus` compute units (<= 0:
 * 256): chunks_out >= 1 with chunks * T * 8 <= 2 MB, and rows_per_chunk_out (a multiple of 32) with
 * chunks * rows_per_chunk >= V > (chunks - 1) * rows_per_chunk.
 *
 * come_kmeans_pp_step: the one pass over x.  cand: device int32 [T], row indices of x.  closest:
 * device fp32 [V], the squared distance to the nearest centre chosen so far, or NULL for +inf (the
 * first centre).  dist_out [V x T] (fp32): dist_out[i][t] = min(closest[i], sum_j (x[i][j] -
 * x[cand[t]][j])^2), the sum taken over the squared differences in fp32 (a candidate's own row
 * gets exactly 0; nothing cancels, nothing is clamped).  ppot [chunks x T] (float64): the column
 * sums of dist_out over each chunk's rows (chunk c = rows c R .. c R + R - 1, R = ceil(V / chunks)
 * rounded up to a multiple of 32: with the planner's chunks, its rows_per_chunk; a chunk past the
 * rows gets 0); pots_out [T] (float64): the sum of ppot's rows in chunk order.  A cand[t] outside
 * [0, V) gives a column of +inf with potential +inf; nothing is read out of bounds.
 *
 * come_kmeans_pp_pick: best = argmin_t pots[t], ties to the lowest t, into best_out (device
 * int32); closest_out[i] = dist[i][best]; cpot_out[c] = ppot[c][best]; pot_out = pots[best]
 * (device float64).
 *
 * come_kmeans_pp_sample: u: device float64 [T], uniform draws in [0, 1).  With pot = the sum of
 * cpot in chunk order and r = u[t] * pot, cand_out[t] (device int32) = the first row i with
 * cum[i] >= r, clamped to V - 1 (a searchsorted), where cum is the float64 cumulative sum of
 * closest: the chunk's prefix of cpot plus the running sum of the chunk's rows.  Whenever pot > 0
 * and u[t] > 0 the row returned has closest > 0 (a chosen centre or a duplicate of one is never
 * drawn again); pot == 0 returns row 0.  cpot and rows_per_chunk are those of the step that
 * produced closest. */
int come_kmeans_pp_scratch(int64_t V, int d, int T, int cus, int *chunks_out,
                           int *rows_per_chunk_out);
int come_kmeans_pp_step(const float *x, int64_t V, int d, const float *closest,
                        const int32_t *cand, int T, int chunks, float *dist_out, double *ppot,
                        double *pots_out, void *stream);
int come_kmeans_pp_pick(const float *dist, int64_t V, int T, const double *ppot,
                        const double *pots, int chunks, float *closest_out, double *cpot_out,
                        int32_t *best_out, double *pot_out, void *stream);
int come_kmeans_pp_sample(const float *closest, int64_t V, const double *cpot, int chunks,
                          int rows_per_chunk, const double *u, int T, int32_t *cand_out,
                          void *stream);

/* ---- Exact top-k neighbour search over an embedding table (come_amd.neighbors) ----
 * q [Q x d] and base [V x d]: device fp32, row-major.  1 <= k <= 64, 1 <= d <= 512, Q >= 1,
 * 1 <= V < 2^31.  metric: COME_TOPK_DOT (q.b, larger is better), COME_TOPK_COSINE (q.b / (|q| |b|);
 * a zero-norm row has inverse norm 0 and scores 0) or COME_TOPK_L2 (max(0, |q|^2 + |b|^2 - 2 q.b),
 * smaller is better).  idx_out int32 [Q x k] and score_out fp32 [Q x k], best first; equal scores
 * in ascending base index; a NaN score is never selected; where fewer than k candidates exist the
 * tail is idx -1, score -inf (+inf for L2).  exclude (optional, device int32 [Q]): the base row
 * query i must not return, -1 for none.  base_sq (optional, device fp32 [V]): come_row_sqnorms of
 * base.  No [Q x V] matrix exists and no float atomics run: bit-identical from run to run.
 *
 * come_topk_scratch (host): the base chunking for a device with `cus` compute units (<= 0: 256):
 * chunks_out <= 64 and rows_per_chunk_out, a multiple of the 32-row base tile with chunks *
 * rows_per_chunk >= V.  The scratch of come_topk (4-byte aligned) is chunks * Q * k * 8 bytes,
 * plus 4 V bytes when base_sq is NULL.  come_topk accepts any chunks in [1, 64].
 *
 * come_row_sqnorms: out[r] = |x_r|^2, an fp32 fmaf chain in feature order.
 *
 * come_cpu_topk: the same contract on host arrays with `threads` threads over the queries (fmaf
 * chains in feature order; on data where the arithmetic is exact, the GPU's bits). */
enum come_topk_metric { COME_TOPK_DOT = 0, COME_TOPK_COSINE = 1, COME_TOPK_L2 = 2 };
int come_topk_scratch(int64_t Q, int64_t V, int d, int k, int cus, int *chunks_out,
                      int64_t *rows_per_chunk_out);
int come_row_sqnorms(const float *x, int64_t V, int d, float *out, void *stream);
int come_topk(const float *q, int64_t Q, const float *base, int64_t V, int d, int k, int metric,
              const int32_t *exclude, const float *base_sq, int chunks, void *scratch,
              int32_t *idx_out, float *score_out, void *stream);
int come_cpu_topk(const float *q, int64_t Q, const float *base, int64_t V, int d, int k,
                  int metric, const int32_t *exclude, const float *base_sq, int32_t *idx_out,
                  float *score_out, int threads);

/* ---- Random walks: the producer of train_o2's input (utils/graph_utils.py) ----
 * Graphs are CSR over node POSITIONS 0..V-1 in networkx order (see come_graph_from_edges):
 * rowptr int64 [V+1], col int32 [rowptr[V]] (neighbours in adjacency order).  `emit` (optional,
 * int32 [V]) maps a position to the value written into a walk (e.g. the node's Vocab.index row);
 * NULL writes positions.  Walk rows are [P x path_length] int32, -1 after a walk ends. */

/* Device walker, same distribution as __random_walk__ (graph_utils.py:20-46): from the current
 * node jump back to the walk's start with probability alpha, else move to a uniform neighbour;
 * a node without neighbours ends the walk.  starts: device int32 [P] positions (one walk per
 * start; build_deepwalk_corpus_iter :187-192 starts one walk at every node per pass, in shuffled
 * order).  Random stream: Philox-4x32-10 keyed by `seed`, counter (walk_offset + walk, step) --
 * independent of launch shape, not the reference's CPython stream.  rowptr/col/emit/out are
 * device pointers. */
int come_random_walks(const int64_t *rowptr, const int32_t *col, int64_t V,
                      const int32_t *starts, int64_t P, int path_length, float alpha,
                      uint64_t seed, int64_t walk_offset, const int32_t *emit, int32_t *out,
                      void *stream);

/* Device walker with node2vec's return / in-out bias (p, q): a second-order walk.  The first
 * step of a walk, and the first after a restart, is come_random_walks' step (same Philox block,
 * same draws); every later step goes from cur (previous node prev) to x in N(cur) with
 * probability proportional to 1/p if x == prev, 1 if x is in N(prev), 1/q otherwise.  Dead ends,
 * restarts (after which the walk has no prev), starts, emit, out, seed and walk_offset as
 * come_random_walks; p = q = 1 gives come_random_walks' walks bit for bit.  A walk depends only
 * on (seed, walk_offset + walk, start, graph, alpha, p, q).  Exact rejection sampling, O(1)
 * expected trials per step (at most 2 max(q, 1/q)), capped: csrc/come_walk_pq.h.
 *   p in [2^-8, 2^8], q in [2^-4, 2^4]; anything else (NaN too) is COME_E_INVALID.
 *   col_sorted: device int32, the rowptr of col with each row ascending (membership searches;
 *     candidates are always drawn from col, so every step is an entry of col's row whatever
 *     col_sorted's order).  May equal col when col's rows are ascending; may be NULL iff q == 1
 *     and p >= 1 (no search runs then).
 *   trials_out: NULL, or one device uint64 to which the launch adds the Philox blocks it drew:
 *     one per step taken plus one per rejected trial (nothing at a dead end).
 * P == 0 or path_length == 0 is a no-op; a validation failure writes nothing.  Asynchronous. */
int come_random_walks_pq(const int64_t *rowptr, const int32_t *col, const int32_t *col_sorted,
                         int64_t V, const int32_t *starts, int64_t P, int path_length,
                         float alpha, float p, float q, uint64_t seed, int64_t walk_offset,
                         const int32_t *emit, int32_t *out, uint64_t *trials_out, void *stream);

/* ---- Edge-weighted walks: a per-row CDF, built once per graph, and the walker over it ----
 * weights: device fp32 [rowptr[V]], entry i the weight w_i >= 0 of CSR entry i.  wcdf_out: device
 * uint32 [rowptr[V]], per entry a cumulative threshold T_i stored minus one; the walker's
 * candidate for a 32-bit uniform r is the first entry i of the row with max(r, 1) <= wcdf[i].
 * Per row, with wmax the row's largest weight:
 *     u_i = llrint((double)w_i / (double)wmax * 2^32)
 *     U_i = u_0 + ... + u_i                       exact, uint64: any order of summation
 *     T_i = min(2^32, ceil((double)U_i / (double)U_last * 2^32)),  T_last = 2^32
 *     wcdf[i] = T_i - 1, and 0 where T_i = 0
 * Division, conversion and ceil are correctly rounded on both sides, so come_walk_cdf and
 * come_cpu_walk_cdf give the same words bit for bit.  Entry i is picked for m_i = wcdf[i] -
 * wcdf[i-1] of the 2^32 values of r (the row's "-1st" threshold taken as -1): |m_i / 2^32 - w_i /
 * sum(w)| is a few units of 2^-32 (at most 3 + (w_i / sum w) * deg * wmax / (2 sum w): the
 * rounding of each u_i, spread over the row).
 * Zero mass: an entry with u_i = 0 (weight 0, or below 2^-33 of the row's largest) repeats its
 * predecessor's threshold and is never picked.  At the head of a row there is no predecessor to
 * repeat: such entries store 0, and the walker never selects a threshold of 0 (it searches for
 * max(r, 1)), so they are never picked either; the value r = 0 goes to the entry that holds
 * r = 1.  A first entry whose own mass is a single unit cedes it to its successor by the same rule.
 * Equal weights: T_i = ceil((i + 1) / deg * 2^32), and the pick is (r * deg) >> 32, the uniform
 * walker's, for every 32-bit r whenever deg < 2^22 (2^32 / deg then exceeds the double rounding
 * of the quotient by far; checked on degrees up to 3,000,001).  Beyond that degree the two picks
 * can differ for isolated r.
 * status: device int32, set to 0 if every row was built, 1 if some weight is NaN, infinite or
 * negative or some row of positive degree has only zero weights; wcdf_out must not be used then
 * (such rows hold 2^32 - 1 throughout).  Rows without entries write nothing.  Asynchronous. */
int come_walk_cdf(const int64_t *rowptr, const float *weights, int64_t V, uint32_t *wcdf_out,
                  int32_t *status, void *stream);

/* come_random_walks_pq over edge weights.  The first step of a walk, the first after a restart and
 * any step from a node of degree 1 go to x in N(cur) with probability w(cur, x) / sum_y w(cur, y);
 * every later step with probability proportional to w(cur, x) * beta, beta = 1/p if x == prev, 1 if
 * x is in N(prev), 1/q otherwise.  Adjacency is what col lists whatever the weight: an entry of
 * weight 0 is never stepped to but counts as a neighbour.  Restarts, dead ends, starts, emit, out,
 * seed, walk_offset, the Philox counters, trials_out and the (p, q) ranges are
 * come_random_walks_pq's; a walk depends only on (seed, walk_offset + walk, start, graph, weights,
 * alpha, p, q).
 *   col: device int32, ONE adjacency array, each row ascending (it serves the membership searches
 *     too, and the return edge's mass is read at prev's index in cur's row); wcdf: come_walk_cdf's
 *     output for the weights in that order.  Neither may be NULL.  A mis-ordered row gives wrong
 *     probabilities but every step is still an entry of the row.
 *   On equal weights and deg < 2^22 the walks are come_random_walks' at p = q = 1 bit for bit.
 *   Expected trials per step: at most max(q, 1/q) * max(1, p) (256 when q >= 1 or p <= 16; 4096
 *   in the corner p = 256, q = 1/16, reached only on rows whose mass sits almost wholly on prev);
 *   at most max(q, 1/q) for p <= 1.  Weaker than the unweighted walker's: csrc/come_walk_pq.h.
 * P == 0 or path_length == 0 is a no-op; a validation failure writes nothing.  Asynchronous. */
int come_random_walks_w(const int64_t *rowptr, const int32_t *col, const uint32_t *wcdf,
                        int64_t V, const int32_t *starts, int64_t P, int path_length, float alpha,
                        float p, float q, uint64_t seed, int64_t walk_offset, const int32_t *emit,
                        int32_t *out, uint64_t *trials_out, void *stream);

/* ---- Edges sampled by weight, for first-order (O1) training on a weighted graph ----
 * The weighted first-order objective sum_e w_e log sigma(x_u . x_v) (+ negatives) is optimised by
 * drawing edges with probability w_e / W, with replacement, and training each draw with the plain
 * come_sgns_o1 step (LINE's edge sampling); these two entries produce the draws.
 *
 * come_edge_cdf.  weights: device fp32 [E], w_i >= 0.  ecdf_out: device uint64 [E].  With wmax the
 * largest weight:
 *     u_i     = llrint((double)w_i / (double)wmax * 2^32)          <= 2^32   (come_walk_cdf's units)
 *     ecdf[i] = U_i = u_0 + ... + u_i                              exact, uint64
 * E must be in [1, 2^31), so U_E < 2^63 and the words fit a signed 64-bit tensor unchanged.  No
 * thresholds and no second rounding: the sums themselves are stored.  Only an order-free maximum
 * and exact integer sums enter, so come_edge_cdf and come_cpu_edge_cdf give the same words bit for
 * bit.  The device scan is four launches (maximum, per-tile totals, scan of the totals by one
 * workgroup, per-tile rescan); no workgroup waits on another.  Uses library scratch on `stream`.
 * Zero mass: an edge with u_i = 0 (weight 0, or below 2^-33 wmax) repeats its predecessor's sum
 * (0 at the head of the array) and is never drawn.
 * status: device int32, set to 0 if the CDF was built, 1 if some weight is NaN, infinite or
 * negative or all weights are zero; ecdf_out must not be used then (its content is unspecified).
 * Asynchronous. */
int come_edge_cdf(const float *weights, int64_t E, uint64_t *ecdf_out, int32_t *status,
                  void *stream);

/* S draws from come_edge_cdf's distribution.  Sample s of the call is global sample gs =
 * sample_offset + s and depends only on (seed, gs, ecdf): a list drawn in pieces with
 * sample_offset = the piece's first index concatenates to the list drawn at once.  gs draws one
 * Philox-4x32-10 block r[0..3] with
 *     counter (gs low 32 bits, gs high 32 bits, 0, 0x45444745)     key (seed low, seed high)
 * -- the walkers' counters (t, gw low, gw high, j) carry a trial index j < 4096 in the last word,
 * so the streams of one seed never meet -- and then
 *     r64  = r[0] << 32 | r[1]
 *     x    = floor(r64 * U_E / 2^64)                               in [0, U_E), U_E = ecdf[E - 1]
 *     pick = the first i with x < ecdf[i]
 * (a search of at most 32 iterations, indices clamped to [0, E)).  Edge i is the pick for
 * ceil(U_i 2^64 / U_E) - ceil(U_{i-1} 2^64 / U_E) of the 2^64 values of r64 (U_{-1} = 0): u_i / U_E
 * to within 2^-64, and |u_i / U_E - w_i / W| <= (1/2 + p_i E / 2) / U_E with p_i = w_i / W, the
 * half-unit rounding of each u_i spread over the total.
 *   edges: device int32 [E, 2], out: device int32 [S, 2], both 8-byte aligned; out[s] =
 *     edges[pick] as given (no orientation draw: O1 trains both directions; rows outside [0, V)
 *     are the trainer's business).  index_out: device int64 [S] = pick, or NULL.
 * S == 0 is a no-op; a validation failure writes nothing.  Asynchronous. */
int come_edge_sample(const int32_t *edges, const uint64_t *ecdf, int64_t E, int64_t S,
                     uint64_t seed, int64_t sample_offset, int32_t *out, int64_t *index_out,
                     void *stream);

/* Host, exact: build_deepwalk_corpus_iter (graph_utils.py:187-192) with the reference's own
 * random stream.  n_streams independent CPython random.Random streams (one per walk file of
 * write_walks_to_disk :122-146); stream s writes paths_per_stream[s] passes of V walks, streams
 * concatenated in order.  states: [n_streams x 625] uint32 = random.Random.getstate()[1] (624
 * MT19937 words + position), advanced in place (setstate() them back to continue the Python
 * streams).  Streams run on up to `threads` host threads.  All pointers are host pointers. */
int come_walks_reference(const int64_t *rowptr, const int32_t *col, int64_t V, int n_streams,
                         const int32_t *paths_per_stream, uint32_t *states, int path_length,
                         double alpha, const int32_t *emit, int threads, int32_t *out);

/* Host: random.Random(seed).getstate()[1] for 0 <= seed < 2^64 (CPython init_by_array). */
int come_pyrandom_seed(uint64_t seed, uint32_t *state625);

/* Host: `count` draws from a CPython random.Random state (advanced in place): kind 0 =
 * random(), kind 1 = _randbelow(arg) (arg <= 2^32).  Test hook for the restated stream. */
int come_pyrandom_draw(uint32_t *state625, int kind, uint64_t arg, int64_t count, double *out);

/* Host: the per-walk / per-edge seeds train_o2 / train_o1 draw from the GLOBAL numpy RNG
 * (pyx:477 / pyx:427: next_random = 2^24 * randint(0, 2^24) + randint(0, 2^24), two draws per
 * call, in call order), for n consecutive calls at once.  state625 = the 624 MT19937 words and
 * the position of numpy.random.get_state() (legacy RandomState: each bounded randint below 2^32
 * consumes one 32-bit output, masked to 24 bits -- the mask equals the range, so nothing is ever
 * rejected), advanced in place (set_state() it back).  out: uint64 [n]. */
int come_np_draw_seeds(uint32_t *state625, int64_t n, uint64_t *out);

/* Host: nx.Graph().add_edges_from(edges) (graph_utils.py:60-69) in networkx order.
 * edges int64 [E x 2] node ids in file order.  Outputs (capacities 2E, 2E+1 for rowptr):
 * node_ids[V] = list(G.nodes()) (first appearance), rowptr/col = adjacency in insertion order
 * (duplicates dropped, a self-loop listed once), degree[V] = G.degree() (self-loop counts 2),
 * edge_pos [E' x 2] = G.edges() as positions, in networkx order. */
int come_graph_from_edges(const int64_t *edges, int64_t E, int64_t *node_ids, int64_t *V_out,
                          int64_t *rowptr, int32_t *col, int64_t *degree, int32_t *edge_pos,
                          int64_t *E_out);

/* ---- Text formats (host) ----
 * Integer rows (edge lists graph_utils.py:49-109, walk files :112-120/:149-154): one row per
 * line of whitespace-separated integers; '#' lines and blank lines skipped.  With rows == NULL
 * only counts (nrows_out, max_tokens_out); else fills rows [cap_rows x width], -1 padded. */
int come_read_int_rows(const char *path, int64_t *rows, int64_t cap_rows, int width,
                       int64_t *nrows_out, int *max_tokens_out);
/* Writes rows [nrows x width] one per line, space separated, each ending at its first
 * negative entry (the walk-file format of _write_walks_to_disk :117-118). */
int come_write_int_rows(const char *path, const int64_t *rows, int64_t nrows, int width,
                        int append);
/* IO_utils.save_embedding (:49-62): "<first_id + i>\t<v1> <v2> ...\n", each value exactly as
 * numpy's str(np.float32) prints it.  emb: host fp32 [V x d]. */
int come_save_embedding(const char *path, const float *emb, int64_t V, int d, int64_t first_id);
/* str(np.float32(x)) into out32 (NUL-terminated); returns its length. */
int come_format_f32(float x, char *out32);

/* ---- Multi-GPU delta exchange (come_amd.distributed.DeltaAllReduce, overlapped) ----
 * Fused elementwise passes around the all-reduce of a replicated table of n floats (device,
 * 16-byte aligned, n % 4 == 0):
 *   come_delta_begin:  D = W - S;  Down = D           (D is then all-reduced in place)
 *   come_delta_end:    S += Dsum;  W += Dsum - Down   (Dsum = the all-reduced D) */
int come_delta_begin(const float *W, const float *S, float *D, float *Down, int64_t n,
                     void *stream);
int come_delta_end(float *W, float *S, const float *Dsum, const float *Down, int64_t n,
                   void *stream);

/* Row-sparse exchange (come_amd.distributed.SparseDeltaAllReduce): only rows some rank changed.
 * W, S: device fp32 [rows x d], d % 4 == 0, 16-byte aligned.
 *   come_delta_flags:   flags[r] = 1 iff row r of W differs bitwise from S, else 0 (uint8 [rows])
 *   come_delta_gather:  D[i] = W[idx[i]] - S[idx[i]]; Down = D    (D, Down: [n x d])
 *   come_delta_scatter: S[idx[i]] += Dsum[i]; W[idx[i]] += Dsum[i] - Down[i]
 * idx: device int64 [n] row indices.  A row no rank changed contributes exactly +0 to the dense
 * exchange, so the sparse one leaves the tables bit-identical to it. */
int come_delta_flags(const float *W, const float *S, int64_t rows, int d, uint8_t *flags,
                     void *stream);
int come_delta_gather(const float *W, const float *S, const int64_t *idx, int64_t n, int d,
                      float *D, float *Down, void *stream);
int come_delta_scatter(float *W, float *S, const int64_t *idx, int64_t n, int d,
                       const float *Dsum, const float *Down, void *stream);

/* ---- Launch options ----
 * Kernel-selection and grid knobs (0 = automatic unless stated):
 *   o2_kernel           1 = direct kernel, 2 = LDS-ring kernel (sequential mode only; Hogwild
 *                       returns COME_E_INVALID), 3 = streaming kernel.  Automatic: sequential ->
 *                       ring when it fits; Hogwild -> streaming when the vocabulary has >= 32 rows
 *                       per wavefront in flight (and window <= 31), else direct
 *   o2_blocks_per_cu    O2 grid cap in workgroups per CU
 *   o2_waves_per_block  1 or 2 (automatic 2)
 *   o2_static           1 = static grid-stride walk assignment instead of the device work queue
 *   rows_per_wave / o1_rows_per_wave  Hogwild launches keep at most V / rows_per_wave
 *                       wavefronts in flight so updates stay sparse on small vocabularies
 *                       (defaults 16 / 12; 0 = no cap)
 *   max_waves           absolute cap on wavefronts in flight (0 = none)
 *   o1_blocks_per_cu    O1 grid cap in 4-wave workgroups per CU (0 = 8 for the run kernel at
 *                       d <= 128, n <= 5 -- compiled for 8 waves per SIMD there -- else 6)
 *   resident_cap        1 = also clamp grids to the workgroups the occupancy API reports resident
 *   community_async     community gradient at d = 64, 128 (16-B aligned mu / inv_cov; else the
 *                       VALU kernel): default 3 = k_community_b16 (each fp32 operand as three
 *                       bf16 parts, six exact part products per multiply-add on 16x16x32 bf16
 *                       MFMAs -- fp32-level error, tests/test_gpu_c4.py; 6.75 vs 11.5 ms at C4);
 *                       2 = k_community16 (fp32 16x16x4 MFMAs, one 16-row tile per wavefront;
 *                       11.5 ms).  Other values: COME_E_INVALID
 *   gmm_cov_async       GMM M-step scatter at d = 64, 128: default 4 = k_gmm_cov_fb3 at d = 128
 *                       (E^T E with E = sqrt(r) (x - m) carried as three bf16 parts, six exact
 *                       part products per multiply-add on 32x32x16 bf16 MFMAs -- four on the
 *                       diagonal tiles, whose cross terms are U + U^T -- the staging inside the
 *                       MFMA wavefronts; 4.6 ms at C4) and k_gmm_cov_bf3 at d = 64 (specialised
 *                       staging wavefronts); 5 = k_gmm_cov_bf3 at both widths (5.5 ms at C4);
 *                       3 = k_gmm_cov16 (fp32 16x16x4 tiles: 36 of 64 upper tiles at d = 128;
 *                       7.22 ms).  Other values: COME_E_INVALID
 *   walk_staged         come_random_walks: default 1 = LDS-staged walker output; 0 = one store per
 *                       lane per step (identical walks).  Other values: COME_E_INVALID
 *   o2_fresh_loads      direct kernel: rows read with agent-scope loads (bypass the CU's L1)
 *   o2_atomic_writeback direct kernel: every row update written as a float-atomic delta
 *   gmm_resp16          GMM E-step at d = 64, 128: default 3 = k_gmm_resp_b16 (fp32 operands
 *                       as three bf16 parts, six exact part products per multiply-add on 16x16x32
 *                       bf16 MFMAs, the row's parts formed once, 4 waves per SIMD; 4.1 ms at
 *                       C4); 2 = k_gmm_resp16t on fp32 16x16x4 MFMAs (16-wide triangular skip,
 *                       in-lane row sums, the factors' non-zero 16x16 blocks packed, whole
 *                       components double-buffered, one barrier per component; 6.95 ms); a
 *                       launch holding a lower or dense factor runs every block, in
 *                       k_gmm_resp16_full, for both.  Other values: COME_E_INVALID
 *   o1_chunk            O1: > 0 = one wavefront per chunk of that many consecutive edges, the
 *                       input row held in registers over each run of edges sharing it
 *                       (k_sgns_o1_runs); default -1 = one contiguous chunk per wavefront of the
 *                       grid (the edges in flight spread over the whole list: tier C holds in
 *                       the reference's G.edges() order, +0.23% vs 1.6% for 0); 0 = one
 *                       wavefront per edge (k_sgns_o1).  Sequential mode: one chunk, in order
 *   o2_update_count     (per call, come_sgns_o2_ex only) device uint64: += the number of target
 *                       row updates the launch applied (positive + negatives that passed the
 *                       +-6 skip, pyx:141-147) -- what the data-dependent part of the O2 HBM
 *                       traffic is counted from.  NULL = not counted. */
typedef struct come_launch_opts {
    int o2_kernel;
    int o2_blocks_per_cu;
    int o2_waves_per_block;
    int o2_static;
    int rows_per_wave;
    int o1_rows_per_wave;
    int max_waves;
    int o1_blocks_per_cu;
    int resident_cap;
    int community_async;
    int gmm_cov_async;
    int walk_staged;
    int o2_fresh_loads;
    int o2_atomic_writeback;
    int gmm_resp16;
    int o1_chunk;
    uint64_t *o2_update_count;
} come_launch_opts;

/* Fills *out with the current process-wide options (o2_update_count = NULL). */
int come_get_options(come_launch_opts *out);

/* Sets one process-wide option by field name (thread-safe; calls already inside the library
 * keep the snapshot they took). */
int come_set_option(const char *name, int value);

/* come_sgns_o2 with the contended-row bitmap and per-call options.
 * hot_rows  device uint32 [ceil(V / 32)] (come_hot_rows), or NULL: in COME_MODE_HOGWILD every
 *           update of a row whose bit is set is a float-atomic delta at the memory side (no
 *           concurrent update lost); O2 also re-reads such a row before each pair (no stale
 *           cached copy), while O1's run kernel (o1_chunk != 0) holds its input row -- hot or
 *           not -- over a run of consecutive edges sharing it and flushes the run's delta once
 *           (atomically when hot: other wavefronts' updates of the row during the run are kept,
 *           the run computes on its own copy; a hot row's delta also goes out before the second
 *           update of a self-loop).  The other rows are written back with plain
 *           stores.  Ignored in COME_MODE_SEQUENTIAL.
 *           NULL: the library derives the bitmap from `table` on `stream` before EVERY launch
 *           (rows holding >= COME_DEFAULT_HOT_SHARE(_WIDE) of the table: a memset of V counters and a
 *           scan of the table, ~0.1 ms at T = 1e8, into library scratch that grows
 *           stream-ordered -- the first call at a larger V allocates, so warm up before capturing
 *           a stream).  Callers that launch many small batches should compute the bitmap once
 *           (come_hot_rows) and pass it; COME_HOT_NONE in `mode` makes every row cold (on graphs
 *           with hubs that trains measurably worse than the reference's Hogwild,
 *           tests/test_gpu_tierc.py).
 * opts      per-call launch options, or NULL = the process-wide ones. */
int come_sgns_o2_ex(float *node, float *ctx, int64_t V, int d, const int32_t *walks, int64_t P,
                    int L, const uint64_t *seeds, int window, int negative,
                    const uint32_t *table, uint64_t T, float lr, float alpha, int mode,
                    const uint32_t *hot_rows, const come_launch_opts *opts, void *stream);

/* Contended rows of a negative-sampling table: counts[v] = number of slots of table[0, T) holding
 * v (device uint32 [V] scratch, overwritten) and hot_bits (device uint32 [ceil(V / 32)]) bit v set
 * iff counts[v] >= min_count.  A row's share of the table is its draw probability as a negative
 * and grows with its count (degree), i.e. with how often walks visit it.  Asynchronous. */
int come_hot_rows(const uint32_t *table, uint64_t T, int64_t V, uint64_t min_count,
                  uint32_t *counts, uint32_t *hot_bits, void *stream);
/* Quiet rows of the node table, for come_sgns_o2_quiet: quiet_bits (device uint32 [ceil(V / 32)])
 * bit v set iff row v is not hot (fewer than hot_min_count slots of the table hold v) and
 *     visitors * share_v <= eps,
 * share_v = row v's share of walk visits = its degree share, recovered from the table: the slots
 * holding the value v + id_shift are sized by row v's count^power (the table stores node ids and
 * the kernels read them as rows, so id_shift = 1 for ids 1..V), hence share_v =
 * counts[v + id_shift]^(1/power) / sum_u counts[u]^(1/power).  A row whose own count the table
 * does not hold (v + id_shift outside [0, V)) is not quiet.  visitors = wavefronts in flight *
 * (2 * window + 1): the product is the expected number of other wavefronts with the row inside
 * their walk window.  counts: device uint32 [V] scratch; sum: device double [1] scratch.
 * Plain (unpacked) table only.  Asynchronous. */
int come_quiet_rows(const uint32_t *table, uint64_t T, int64_t V, double power, int id_shift,
                    double visitors, double eps, uint64_t hot_min_count, uint32_t *counts,
                    double *sum, uint32_t *quiet_bits, void *stream);
/* come_sgns_o2_ex with a quiet-row bitmap (come_quiet_rows), or NULL = come_sgns_o2_ex.  Where
 * the Hogwild launch runs the streaming kernel with d <= 128, negative <= 5, window <= 5 and
 * V < 2^30, a quiet input row is read once when a walk position holding it enters the
 * wavefront's window and written back once when the last such position leaves it (an LDS ring
 * per wavefront), instead of once per pair; other wavefronts' updates of the row during the
 * stay are overwritten.  With one wavefront the results are bit-identical to come_sgns_o2_ex.
 * Every other shape, kernel and mode ignores the bitmap.  Default grid there: 5 four-wave
 * workgroups per CU (o2_blocks_per_cu = 0). */
int come_sgns_o2_quiet(float *node, float *ctx, int64_t V, int d, const int32_t *walks, int64_t P,
                       int L, const uint64_t *seeds, int window, int negative,
                       const uint32_t *table, uint64_t T, float lr, float alpha, int mode,
                       const uint32_t *hot_rows, const uint32_t *quiet_rows,
                       const come_launch_opts *opts, void *stream);
/* come_sgns_o1 with the contended-row bitmap (Hogwild: an update of a hot endpoint row is a
 * float-atomic delta; NULL = derived from the table, COME_HOT_NONE = none, as come_sgns_o2_ex)
 * and per-call options (opts may be NULL = process-wide). */
int come_sgns_o1_ex(float *node, int64_t V, int d, const int32_t *edges, int64_t E,
                    const uint64_t *seeds, int negative, const uint32_t *table, uint64_t T,
                    float lr, int mode, const uint32_t *hot_rows, const come_launch_opts *opts,
                    void *stream);

/* ---- CPU twins: the same computations on HOST memory with `threads` worker
 * threads (1..1024), in come_cpu.cpp.  Separate entry points for callers without a GPU; no GPU
 * entry point calls them (no fallback).  Same argument meaning and validation as the GPU entry
 * points above; the uint32 table only (no COME_TABLE_PACKED); pairs_out (may be NULL) receives
 * the pair updates performed.
 *  come_cpu_sgns_o2 / _o1  COME_MODE_HOGWILD: `threads` workers take jobs of 150 walks (edges) and
 *                          update the shared tables without locks, as the reference's Context2Vec /
 *                          Node2Vec worker threads (context_embeddings.py:72-102,
 *                          node_embeddings.py:58-95); COME_MODE_SEQUENTIAL: the calling thread, in
 *                          order (= workers=1), bit-identical to come_sgns_o2 / _o1 sequential
 *                          mode (the same WAVE64 dot order).
 *  come_cpu_community_grad community_embeddings.py:61-78, k_community_grad's arithmetic order.
 *  come_cpu_gmm_resp / _estep  community_embeddings.py:37 predict_proba; _estep adds lse_out.
 *  come_cpu_community_loss come_community_loss in float64 arithmetic (row_out [V] fp32 or NULL,
 *                          loss_out one host double); the total is summed per thread block of rows,
 *                          so it is reproducible for a given `threads`.
 *  come_cpu_sgns_o2_loss / _pairs_loss  come_sgns_o2_loss / come_sgns_pairs_loss on host pointers
 *                          (no flags: the uint32 table): the same dot, float64 softplus and
 *                          summation order, so the per-walk / per-pair values differ from the
 *                          GPU's by the two libms only and do not depend on `threads`; the total
 *                          is summed per thread block of walks (pairs), so it is reproducible for
 *                          a given `threads`.  pairs_out: one host int64 or NULL. */
int come_cpu_sgns_o2(float *node, float *ctx, int64_t V, int d, const int32_t *walks, int64_t P,
                     int L, const uint64_t *seeds, int window, int negative, const uint32_t *table,
                     uint64_t T, float lr, float alpha, int mode, int threads, int64_t *pairs_out);
int come_cpu_sgns_o1(float *node, int64_t V, int d, const int32_t *edges, int64_t E,
                     const uint64_t *seeds, int negative, const uint32_t *table, uint64_t T,
                     float lr, int mode, int threads, int64_t *pairs_out);
int come_cpu_community_grad(float *x, int64_t V, int d, const float *pi, const float *mu,
                            const float *inv_cov, int K, float beta, float lr, int iters,
                            int threads);
int come_cpu_gmm_resp(const float *x, int64_t V, int d, const float *prec_chol,
                      const float *mu_prec, const float *log_norm, int K, float *resp_out,
                      int threads);
int come_cpu_gmm_estep(const float *x, int64_t V, int d, const float *prec_chol,
                       const float *mu_prec, const float *log_norm, int K, float *resp_out,
                       float *lse_out, int threads);
int come_cpu_community_loss(const float *x, int64_t V, int d, const float *pi,
                            const float *prec_chol, const float *mu_prec, const float *log_norm,
                            int K, float *row_out, double *loss_out, int threads);
int come_cpu_sgns_o2_loss(const float *node, const float *ctx, int64_t V, int d,
                          const int32_t *walks, int64_t P, int L, const uint64_t *seeds,
                          int window, int negative, const uint32_t *table, uint64_t T,
                          double *walk_out, double *loss_out, int64_t *pairs_out, int threads);
int come_cpu_sgns_pairs_loss(const float *inp, const float *out, int64_t V, int d,
                             const int32_t *rows_in, const int32_t *rows_pos,
                             const int32_t *rows_neg, int64_t M, int negative, double *pair_out,
                             double *loss_out, int64_t *pairs_out, int threads);
/* come_random_walks_pq on host pointers (trials_out: one host uint64, added to, or NULL): the
 * kernel's own step body (csrc/come_walk_pq.h), so the walks and the trial count are the
 * device's bit for bit, whatever `threads`. */
int come_cpu_random_walks_pq(const int64_t *rowptr, const int32_t *col, const int32_t *col_sorted,
                             int64_t V, const int32_t *starts, int64_t P, int path_length,
                             float alpha, float p, float q, uint64_t seed, int64_t walk_offset,
                             const int32_t *emit, int32_t *out, uint64_t *trials_out,
                             int threads);
/* come_walk_cdf and come_random_walks_w on host pointers (status_out: one host int32, written;
 * trials_out: one host uint64, added to, or NULL): the same arithmetic and the same step body,
 * so wcdf, status, walks and trial count are the device's bit for bit, whatever `threads`. */
int come_cpu_walk_cdf(const int64_t *rowptr, const float *weights, int64_t V, uint32_t *wcdf_out,
                      int32_t *status_out, int threads);
int come_cpu_random_walks_w(const int64_t *rowptr, const int32_t *col, const uint32_t *wcdf,
                            int64_t V, const int32_t *starts, int64_t P, int path_length,
                            float alpha, float p, float q, uint64_t seed, int64_t walk_offset,
                            const int32_t *emit, int32_t *out, uint64_t *trials_out, int threads);
/* come_edge_cdf and come_edge_sample on host pointers (status_out: one host int32, written; no
 * alignment requirement): the same arithmetic and the same draw, so ecdf, status, rows and indices
 * are the device's bit for bit, whatever `threads`.  On status 1 ecdf_out is left untouched. */
int come_cpu_edge_cdf(const float *weights, int64_t E, uint64_t *ecdf_out, int32_t *status_out,
                      int threads);
int come_cpu_edge_sample(const int32_t *edges, const uint64_t *ecdf, int64_t E, int64_t S,
                         uint64_t seed, int64_t sample_offset, int32_t *out, int64_t *index_out,
                         int threads);
/* Test support: idx_out[k] = the sampler's pick for the 64-bit uniform r64[k] (the r64 above in
 * place of a Philox draw), k < n. */
int come_cpu_edge_pick(const uint64_t *ecdf, int64_t E, const uint64_t *r64, int64_t n,
                       int64_t *idx_out);

/* ---- Host helpers ---- */

/* Model.make_table (model.py:97-122), exact: same double accumulation, same start at node id 1,
 * same clamp.  counts_by_id[0..V] (index 0 unused), table[T] (host memory).  O(V + T). */
int come_make_table(const double *counts_by_id, int64_t V, uint32_t *table, uint64_t T,
                    double power);

/* Host: the rows of `count` consecutive negative draws from next_random = seed (pyx:133-134:
 * table[(nr >> 16) % T], then the LCG step), i.e. every row the walk's (edge's) negatives can
 * touch: a train_o2 call on a walk with p pairs draws p * negative, train_o1 2 * negative. */
int come_lcg_table_draws(uint64_t seed, int64_t count, const uint32_t *table, uint64_t T,
                         uint32_t *out);

/* Number of pair updates train_o2 performs on host walks [P x L] (-1 = None). */
int64_t come_count_o2_pairs(const int32_t *walks, int64_t P, int L, int window);

#ifdef __cplusplus
}
#endif

#endif /* COME_H_ */
