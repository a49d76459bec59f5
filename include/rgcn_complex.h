/* rgcn_complex.h - the ComplEx edge-scoring head of librgcn_hip.so (plain C, gfx950 only).
 *
 * The error codes, the ABI version, the alignment rule and the conventions (device pointers, `stream` a hipStream_t
 * passed as void*, asynchronous, no allocation, no host synchronisation, nothing aborts) are those of rgcn_hip.h.  The
 * operand convention is the DistMult head's: a matrix plus an optional int64 index vector; a NULL index means "row b
 * of the matrix is sample b's row", and `*_rows` is the number of rows of the matrix.
 *
 * Layout: a row of width d (a multiple of 8) is m = d / 2 complex numbers; columns [0, m) hold the real parts and
 * columns [m, d) the imaginary parts.  Entity rows and relation rows share the layout.
 *
 * Score, with this grouping (the grouping is part of the contract):
 *
 *   score(h, r, t) = Re <h, r, conj(t)>
 *                  = sum_j (h_re r_re - h_im r_im)_j t_re_j + (h_re r_im + h_im r_re)_j t_im_j
 *
 * The score is NOT symmetric in h and t: the tail enters conjugated.
 *
 * Gradients per sample, with g = d loss / d score:
 *
 *   gh_re = g (r_re t_re + r_im t_im)    gh_im = g (r_re t_im - r_im t_re)
 *   gt_re = g (h_re r_re - h_im r_im)    gt_im = g (h_re r_im + h_im r_re)
 *   gr_re = g (h_re t_re + h_im t_im)    gr_im = g (h_re t_im - h_im t_re)
 *
 * Rules carried over from the DistMult head:
 *   - an id outside its table is clamped to row 0 before use and raises the sticky flag (rgcn_index_error_fetch);
 *   - pointers: tables, gradients, q and the workspace at 16 bytes, index vectors at 8, per-sample vectors and
 *     scalars at 4 (RGCN_ERR_ALIGN, checked after every other argument check and before the first HIP call);
 *   - d <= 0 or d & 7 is RGCN_ERR_ARG;
 *   - batch == 0 with valid sizes is RGCN_OK before any pointer is looked at (the backward still clears the gradient
 *     tables when zero_tables is set);
 *   - non-finite values: plain fp32 arithmetic, rule 10 of rgcn_hip.h - the non-finite sets of scores, losses and
 *     gradients are float64's entry by entry FOR THE GROUPING ABOVE, and rows no sample names stay exact zeros;
 *   - every sum has a fixed order and there are no floating-point atomics: two calls give the same bits;
 *   - the first call on a device looks up the address of the sticky flag, which is not a stream operation: make one
 *     eager call per device before capturing these entry points into a HIP graph.
 *
 * distmult_bce_reduce (rgcn_hip.h) is decoder-independent: it forms the mean of complex_bce_fwd's per-sample losses.
 */
#ifndef RGCN_COMPLEX_H
#define RGCN_COMPLEX_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* scores[b] = score(H[hi(b)], R[ri(b)], T[ti(b)]), float[batch]. */
int complex_fwd(const float* h, const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx,
                int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows, int64_t batch, int64_t d,
                float* scores, void* stream);

/* complex_fwd plus loss[b] = binary_cross_entropy_with_logits(scores[b], labels[b]) in the same launch. */
int complex_bce_fwd(const float* h, const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx,
                    int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows, const float* labels,
                    int64_t batch, int64_t d, float* scores, float* loss, void* stream);

/* Bytes of workspace the two backward entry points need; r_rows: the rows of the relation matrix when it is read
 * through an index vector, else 0.  0 for an empty batch. */
size_t complex_bwd_workspace_bytes(int64_t batch, int64_t d, int64_t r_rows);

/* The gradients of the three operands for grad_scores float[batch].  An operand WITHOUT an index: row b of its
 * gradient buffer is written with sample b's gradient row.  An operand WITH an index: every row some sample names is
 * WRITTEN with the sum of its samples' rows in sample order (the relation table: per segment of the batch, then over
 * the segments); the rows nobody names are cleared by the first launch when zero_tables is set, otherwise they keep
 * what the caller put there (the relation table is always written whole).  grad_h == grad_t with both operands
 * indexed is ONE table and one key space: head slots, then tail slots.  A NULL gradient is not computed.
 * RGCN_ERR_WORKSPACE: workspace NULL or smaller than complex_bwd_workspace_bytes says.
 * RGCN_ERR_UNSUPPORTED: batch > (2^31 - 1) / 4 or a table of more than 2^31 - 1 rows (the keys are int32). */
int complex_bwd(const float* grad_scores, const float* h, const int64_t* h_idx, int64_t h_rows, const float* t,
                const int64_t* t_idx, int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows,
                int64_t batch, int64_t d, float* grad_h, float* grad_t, float* grad_r, void* workspace,
                size_t workspace_bytes, int zero_tables, void* stream);

/* complex_bwd for the mean BCE loss: g_b = grad_mean_loss[0] * (sigmoid(scores[b]) - labels[b]) / batch. */
int complex_bce_bwd(const float* grad_mean_loss, const float* scores, const float* labels, const float* h,
                    const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx, int64_t t_rows,
                    const float* r, const int64_t* r_idx, int64_t r_rows, int64_t batch, int64_t d, float* grad_h,
                    float* grad_t, float* grad_r, void* workspace, size_t workspace_bytes, int zero_tables,
                    void* stream);

/* The query rows that make the score linear in the candidate: score = <q[b], E[n]> for every entity row E[n].
 * One launch gathers x and rel and rotates; q is float[batch, d].
 *   side 0, the tails of (x, rel, ?):  q = [x_re r_re - x_im r_im | x_re r_im + x_im r_re]
 *   side 1, the heads of (?, rel, x):  q = [r_re x_re + r_im x_im | r_re x_im - r_im x_re]
 * The two differ: the head-side operand carries the conjugate.  Any other side is RGCN_ERR_ARG. */
int rgcn_complex_query(int side, const float* x, const int64_t* x_idx, int64_t x_rows, const float* rel,
                       const int64_t* rel_idx, int64_t rel_rows, int64_t batch, int64_t d, float* q, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_COMPLEX_H */
