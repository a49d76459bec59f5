/* rgcn_transe.h - one batch-synchronous training step of the TransE baseline of librgcn_hip.so (plain C, gfx950 only).
 *
 * The error codes, the ABI version and the conventions (device pointers, `stream` a hipStream_t passed
 * as void*, asynchronous, no allocation, nothing aborts) are those of rgcn_hip.h - with ONE exception: the two tables
 * `emb` and `rel` are updated IN PLACE.
 *
 * Replaces the body of the reference's `SimpleTransE.fit` batch loop (src/compare_methods.py:229-270): the two scores,
 * the margin loss, the per-sample Python loop of row updates and the renormalisation of the entity table.
 */
#ifndef RGCN_TRANSE_H
#define RGCN_TRANSE_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace rgcn_transe_step needs for this shape (0 for an empty batch or a shape it rejects). */
size_t rgcn_transe_step_workspace_bytes(int64_t batch, int64_t d, int64_t num_relations);

/* One step over `batch` positives and their `batch` corruptions.
 *
 * emb float[num_nodes, d] and rel float[num_relations, d] are the entity table E and the relation table R.  heads,
 * tails and rels are int64[2 * batch] in the layout rgcn_sample_batch(..., num_neg = 1) writes: entries [0, B) are the
 * positives (h_i, t_i, r_i), entry B + i is the corruption (h'_i, t'_i) of positive i; its relation is r_i (rels[B + i]
 * is not read).
 *
 * Contract, for i in [0, B), all in fp32, every difference from the tables AS THEY STAND WHEN THE STEP BEGINS:
 *   - dp_i = (E[h_i] + R[r_i]) - E[t_i],  dn_i = (E[h'_i] + R[r_i]) - E[t'_i].
 *   - x_i = margin + |dp_i| - |dn_i| (Euclidean norms); loss_i = x_i when x_i > 0, 0 when x_i <= 0, NaN when x_i is NaN.
 *   - sample i is ACTIVE when x_i > 0; a NaN x_i is not active (the reference's `loss[i] > 0`), but makes loss_mean NaN.
 *   - slots: sample i owns slots 4i .. 4i + 3 = (positive head, positive tail, negative head, negative tail) with the
 *     contributions -2 lr dp_i, +2 lr dp_i, +2 lr dn_i, -2 lr dn_i.  Entity row x gains the sum, taken in slot order
 *     from zero, of the contributions of the slots of ACTIVE samples that name it, and is then divided by its Euclidean
 *     norm - no epsilon, as in the reference: a row that becomes zero becomes non-finite.
 *   - an entity row that no active slot names keeps its bits (the reference renormalises every row every batch; those
 *     rows are unit length to rounding already).
 *   - R[r] -= the sum of 2 lr (dp_i - dn_i) over the active samples with r_i = r: per segment of the batch in sample
 *     order, then over the segments in order (the tree of rgcn_segment_sum); an inactive sample adds an exact zero.
 *     Relation rows are never renormalised, as in the reference.
 *   - loss_mean[0] = (sum of loss_i in a fixed order) / B is written; loss_sum[0] += loss_mean[0] (as a double) and
 *     active_sum[0] += the number of active samples accumulate over calls: one read-back per epoch.  Either of the two
 *     accumulators may be NULL.
 *   - every sum has a fixed order and there are no floating-point atomics: two calls from the same tables give the
 *     same bits.
 *   - duplicates are the rule: a tail-corrupted sample has h'_i = h_i; h_i = t_i is legal; so is a corruption equal to
 *     its positive (loss_i = margin; when active its contributions cancel up to rounding and the rows are renormalised).
 *   - an index outside its table is clamped to row 0 before use and raises the sticky flag (rgcn_index_error_fetch).
 *   - the synchronous update scales a row that occurs m times by about 1 - 2 lr m before the normalisation: keep
 *     2 lr m < 1 for the busiest node of a batch.  Not enforced.
 *
 * RGCN_ERR_ARG: batch < 0, d <= 0, d & 3, num_nodes <= 0, num_relations <= 0; with batch > 0: emb, rel, heads, tails,
 * rels, loss_mean or workspace NULL, or workspace_bytes smaller than rgcn_transe_step_workspace_bytes says.
 * batch == 0 (with valid sizes): RGCN_OK before any pointer is looked at; nothing is written, loss_mean included.
 * RGCN_ERR_UNSUPPORTED: num_nodes or num_relations > 2^31 - 1 (the keys are int32), batch > 2^28. */
int rgcn_transe_step(float* emb, int64_t num_nodes, float* rel, int64_t num_relations, int64_t d,
                     const int64_t* heads, const int64_t* tails, const int64_t* rels, int64_t batch,
                     float lr, float margin, float* loss_mean, double* loss_sum, int64_t* active_sum,
                     void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_TRANSE_H */
