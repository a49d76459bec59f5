/* rgcn_sampling.h - protocol-aware batch sampling of librgcn_hip.so (plain C, gfx950 only).
 *
 * The error codes, the ABI version and the conventions (device pointers, `stream` a hipStream_t passed
 * as void*, asynchronous, no allocation, nothing aborts) are those of rgcn_hip.h.
 */
#ifndef RGCN_SAMPLING_H
#define RGCN_SAMPLING_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rgcn_sample_batch with type-constrained and filtered negatives: one launch, one thread per output sample.
 * The slice, cursor, order and rng arguments and the four outputs are rgcn_sample_batch's.  Three optional
 * groups follow; a group whose pointers are all NULL is switched off, a half-given group is RGCN_ERR_ARG.
 *
 *   classes  class_of int32[num_nodes] (-1: no class), class_ptr int64[num_classes + 1], class_members int64
 *            [class_ptr[num_classes]]: the node ids of every class, ascending within a class.
 *   known    per side the CSR of the known triples: keys int64[num_keys] (the sorted anchor * num_relations +
 *            relation that occur), ptr int64[num_keys + 1], ids int64[nnz] ascending per segment.  Side "tail" is
 *            keyed by (head, relation) and lists tails; side "head" is keyed by (tail, relation) and lists heads.
 *   stats    int64[2] = {rejected draws, negatives that gave up}; the launch ADDS to it (integer atomics after
 *            a per-wave sum, so the totals do not depend on launch order).
 *
 * Contract:
 *   - Positives, relations, labels, the clamping of a window past the end and ctr = (cursor + p) * num_neg + j
 *     are exactly rgcn_sample_batch's.
 *   - Block t, t = 0 .. max_tries - 1, is Philox4x32-10 with key = the two halves of the seed and counter
 *     (ctr_lo, ctr_hi, epoch_lo, epoch_hi XOR (t << 24)).  Block 0 is rgcn_sample_batch's block.  Epochs must
 *     stay below 2^56: bits 56..59 carry the try.
 *   - Side: the top bit of word 0 of block 0.  Set: the head is replaced, the anchor is the tail and the known
 *     side is "head".  Clear: the tail is replaced, the anchor is the head and the known side is "tail".
 *   - Candidate of try t, w = word 1 of block t.  No classes: (w * num_nodes) >> 32.  With classes, c =
 *     class_of[replaced node]: c < 0 or class c empty -> (w * num_nodes) >> 32, otherwise
 *     class_members[class_ptr[c] + ((w * size_c) >> 32)].
 *   - The first accepted candidate wins.  A candidate is accepted when no known set is given or (anchor,
 *     relation, candidate) is not in it: a binary search of keys for anchor * num_relations + relation, then one
 *     of that segment's ids.  Every rejected draw adds 1 to stats[0].
 *   - If all max_tries draws are rejected the last candidate is kept and stats[1] gains 1.
 *   - With all three groups NULL and max_tries = 1 the output equals rgcn_sample_batch's bit for bit.
 *
 * RGCN_ERR_ARG: a negative size, num_nodes <= 0, max_tries outside 1..16, a half-given group, a NULL output or
 * graph array.  RGCN_ERR_UNSUPPORTED: num_nodes > 2^32.  batch * (1 + num_neg) == 0: RGCN_OK, nothing launched. */
int rgcn_sample_batch_constrained(const int64_t* edge_index, const int64_t* edge_type, int64_t num_edges,
                                  const int64_t* order, const int64_t* cursor, int64_t batch, int64_t num_neg,
                                  int64_t num_nodes, const int64_t* rng,
                                  const int32_t* class_of, const int64_t* class_ptr, const int64_t* class_members,
                                  int64_t num_classes,
                                  const int64_t* tail_keys, const int64_t* tail_ptr, const int64_t* tail_ids,
                                  int64_t tail_num_keys, int64_t tail_nnz,
                                  const int64_t* head_keys, const int64_t* head_ptr, const int64_t* head_ids,
                                  int64_t head_num_keys, int64_t head_nnz, int64_t num_relations,
                                  int max_tries, int64_t* stats,
                                  int64_t* heads, int64_t* tails, int64_t* rels, float* labels, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_SAMPLING_H */
