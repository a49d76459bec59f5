/* rgcn_tsne.h - t-SNE projection of embedding rows to the plane, of librgcn_hip.so (plain C, gfx950 only).
 *
 * The reference's visualize_embeddings.reduce_dimensions: TSNE(n_components = 2, perplexity = min(30, n - 1),
 * max_iter = 1000) - scikit-learn's neighbour-based pipeline with EXACT repulsion (what scikit-learn computes at
 * angle = 0; its default is the Barnes-Hut approximation at angle = 0.5).  Exact repulsion is O(M^2) per iteration.
 *
 * The error codes, the ABI version and the conventions (device pointers, `stream` a hipStream_t passed as void*,
 * asynchronous, no allocation, nothing aborts, every argument check before any launch) are those of rgcn_hip.h.
 * There are no floating-point atomics: every sum is formed in an order fixed by the shapes (and `slices`) alone, the
 * same inputs give the same bits on every call.  n_components is 2 throughout: y is float32[M, 2].
 */
#ifndef RGCN_TSNE_H
#define RGCN_TSNE_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGCN_KNN_MAX_K 127

/* Finishes the k nearest neighbours of every row from k + 1 candidates per row (the selection itself is
 * distmult_topk_masked on augmented rows: descending <x_i, x_j> - |x_j|^2 / 2 is ascending |x_i - x_j|^2 for a fixed i).
 *   x float32[M, d] contiguous, d % 4 == 0; cand int64[M, k + 1], 1 <= k <= RGCN_KNN_MAX_K, k + 1 <= M
 *   - the row's own id is dropped if it is among its candidates, else the LAST candidate is (more than k duplicates
 *     of the row exist);
 *   - sqdist is recomputed for the k kept pairs from the DIFFERENCES, an fp32 fmaf chain over the columns in order:
 *     equal rows are at distance exactly 0;
 *   - the row is ordered by (sqdist, id) ascending (a NaN distance orders as +inf).
 * ids int32[M, k], sqdist float32[M, k].  A candidate id outside [0, M) comes back as id -1 with sqdist +inf.
 * RGCN_ERR_ARG: M < 2, d <= 0, k < 1, k + 1 > M, a NULL array.  RGCN_ERR_UNSUPPORTED: d % 4 != 0, k above the cap,
 * M >= 2^24. */
int rgcn_knn_refine(const float* x, int64_t M, int64_t d, const int64_t* cand, int64_t k, int32_t* ids, float* sqdist,
                    void* stream);

/* Conditional affinities of every row over its k neighbours: scikit-learn's _binary_search_perplexity, in double,
 * one row at a time.  sqdist float32[M, k] (2 <= k <= RGCN_KNN_MAX_K), 0 < perplexity < k.
 *   beta = 1, bounds -inf / +inf, at most 100 steps:  p_j = exp(-D_j beta), s = sum p (s == 0: s = 1e-8),
 *   H = log s + beta sum D_j p_j / s;  stop when |H - log(perplexity)| <= 1e-5;  H above: beta doubles (or goes half way
 *   to the upper bound once there is one);  below: beta halves (or goes half way to the lower bound).
 * cond_p float32[M, k] = p_j / s of the last step, beta float32[M].
 * RGCN_ERR_ARG: M < 1, k < 2, perplexity not in (0, k) or NaN, a NULL array.  RGCN_ERR_UNSUPPORTED: k above the cap. */
int rgcn_tsne_affinities(const float* sqdist, int64_t M, int64_t k, double perplexity, float* cond_p, float* beta,
                         void* stream);

/* Bytes of workspace rgcn_tsne_gradient and rgcn_tsne_update need (one size serves both); 0 for arguments they
 * refuse.  slices as below. */
size_t rgcn_tsne_workspace_bytes(int64_t M, int64_t slices);

/* One gradient of the Kullback-Leibler objective at the layout y float32[M, 2], 2 <= M < 2^24.
 * P is symmetric CSR: rowptr int32[M + 1] non-decreasing from 0 to nnz < 2^31, col int32[nnz] in [0, M) ascending within
 * a row, val float32[nnz].  A row may have any length up to M - 1.
 *   q_ij   = 1 / (1 + |y_i - y_j|^2)   in fp32 from the DIFFERENCES (never from the Gram form: late layouts have
 *            near-coincident points and that form's error is relative to |y|^2)
 *            as IEEE arithmetic gives it: two rounded squares, their rounded sum, 1 + that, a correctly rounded quotient
 *            (the all-pairs pass takes the hardware reciprocal and two Newton steps, which rounds correctly unless the
 *            significand of 1 + |y_i - y_j|^2 is all ones - then it may be one ulp off).  |y_i - y_j|^2 must be finite
 *            for every pair (|y| below about 1e19): past that the all-pairs pass yields NaN where 1 / inf is 0
 *   Z      = sum over i != j of q_ij   per row and per 256 columns [256 t, 256 t + 256) eight fp32 chains - chain u takes
 *            columns u, u + 8, ... of the block in order - added as ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7));
 *            the blocks of a row, and the rows, in double
 *   rep_i  = sum over j != i of q_ij^2 (y_i - y_j)
 *   attr_i = sum over j in row i of p_ij q_ij (y_i - y_j)      entries in column order
 *   grad_i = 4 (exaggeration attr_i - rep_i / Z)               float32[M, 2]
 *   kl     = sum over nnz of p' log(max(p', FLT_MIN) / max(q_ij / Z, FLT_MIN)),  p' = exaggeration p, in double
 *            (only when compute_error != 0; otherwise kl is not written)
 * z double[1], kl double[1].  slices: workgroups that share one 256-row tile of the repulsion (they divide the
 * columns in units of 256); 0: chosen from M (about four workgroups per compute unit); at most 64 are used.  For a
 * given slices the outputs are the same bits on every call; across slice counts they agree to rounding.
 * RGCN_ERR_ARG: M < 2, nnz < 0, slices < 0, exaggeration not finite or <= 0, a NULL array, a NULL or short workspace.
 * RGCN_ERR_UNSUPPORTED: M >= 2^24, nnz >= 2^31. */
int rgcn_tsne_gradient(const float* y, int64_t M, const int32_t* rowptr, const int32_t* col, const float* val, int64_t nnz,
                       float exaggeration, int64_t slices, int compute_error, float* grad, double* z, double* kl,
                       void* ws, size_t ws_bytes, void* stream);

/* One step of scikit-learn's _gradient_descent, elementwise over the 2 M entries, fp32, in place:
 *   inc = update * grad < 0;  gains += 0.2 where inc, gains *= 0.8 elsewhere;  gains = max(gains, min_gain)
 *   g = grad * gains;  update = momentum * update - learning_rate * g;  y += update
 *   grad_norm2 double[1] = sum of g^2, in double, in a fixed order
 * (a launch of its own: the gradient reads every y_j).  ws_bytes >= rgcn_tsne_workspace_bytes(M, any slices).
 * RGCN_ERR_ARG: M < 2, a NULL array, a NULL or short workspace, a NaN momentum / learning_rate / min_gain.
 * RGCN_ERR_UNSUPPORTED: M >= 2^24. */
int rgcn_tsne_update(const float* grad, int64_t M, float momentum, float learning_rate, float min_gain, float* y,
                     float* update, float* gains, double* grad_norm2, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_TSNE_H */
