/* rgcn_paths.h - score-ranked connecting paths between node pairs of librgcn_hip.so (plain C, gfx950 only).
 *
 * The error codes, the ABI version and the conventions (device pointers, `stream` a hipStream_t passed
 * as void*, asynchronous, no allocation, nothing aborts) are those of rgcn_hip.h.
 */
#ifndef RGCN_PATHS_H
#define RGCN_PATHS_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The structure all three calls read is the node-level digraph of a relational graph, as two CSRs over the UNIQUE
 * (src, dst) pairs (nnz of them):
 *   out_ptr int64[num_nodes + 1], out_dst int32[nnz]   the pairs by src, then dst ascending
 *   in_ptr  int64[num_nodes + 1], in_src  int32[nnz]   the same pairs by dst, then src ascending
 *   in_pos  int64[nnz]                                 the position of every in-entry in the out arrays
 * Self loops may be present.  num_nodes < 2^31. */

/* edge_score[e] = <x_u, x_v> / (|x_u| * |x_v|) of the e-th out-entry (u, v), rows of emb float32[num_nodes, d],
 * accumulated in fp32; a zero norm gives 0.0.
 * RGCN_ERR_ARG: d <= 0, num_nodes <= 0, nnz < 0, a NULL array with nnz > 0.  RGCN_ERR_UNSUPPORTED: d % 32 != 0,
 * num_nodes >= 2^31.  nnz == 0: RGCN_OK, nothing launched. */
int rgcn_edge_cosine(const float* emb, int64_t num_nodes, int d, const int64_t* out_ptr, const int32_t* out_dst,
                     int64_t nnz, float* edge_score, void* stream);

/* Bytes of workspace rgcn_paths_topk needs; 0 for num_queries <= 0, k outside 1..64 or slices < 0. */
size_t rgcn_paths_workspace_bytes(int64_t num_queries, int k, int slices);

/* The k best-scoring simple paths of at most max_len edges from sources[q] to targets[q], and how many there are of
 * every length, for num_queries queries.
 *
 * Contract:
 *   - A path of length L is a node sequence s = n0 -> n1 -> ... -> nL = t with every consecutive pair in the
 *     structure and all L + 1 nodes distinct, 1 <= L <= max_len, max_len in 1..4.  s == t has no paths.
 *   - score = (((c1 + c2) + c3) + c4)[the first L terms] * w[L]: c_i the edge_score of hop i, w[L] =
 *     (float)(1.0 / (L * (1 + 0.2 * (L - 1)))), every operation in fp32, in exactly this order, nothing contracted
 *     into a fused multiply-add: a host restates the score bit for bit from edge_score.  (The mean of the hops'
 *     scores times the length penalty 1 / (1 + 0.2 * (nodes - 2)).)
 *   - count int64[Q, 4]: count[q, L - 1] is the exact number of simple paths of length L (0 for L > max_len).  A path
 *     whose score is NaN is counted: edge_score is the caller's.
 *   - Selected are the k best paths whose score is not NaN under the total order: score descending, then L
 *     ascending, then (n1, n2, n3) lexicographically ascending.  The result does not depend on slices, on how the
 *     waves are scheduled or on the order in which paths are found.
 *   - nodes int32[Q, k, 5]: row j of query q is n0 .. nL of its j-th best path, -1 past nL; length int32[Q, k] its L;
 *     score float32[Q, k].  Slots past the number of paths: nodes -1, length 0, score -inf.
 *   - k in 1..64 (one list entry per lane of a wave).
 *   - slices: the number of workgroups that share one query (they divide its (first hop, second hop) prefixes); 0:
 *     chosen from num_queries so that a small batch still fills the device; at most 256 are used.
 *   - A source or target outside [0, num_nodes): that query has zero counts and empty slots; nothing is read for it.
 *
 * RGCN_ERR_ARG: num_queries < 0, num_nodes <= 0, nnz < 0, max_len outside 1..4, k <= 0, slices < 0; with
 * num_queries > 0: a NULL array (out_dst / edge_score / in_src / in_pos may be NULL when nnz == 0), a NULL or short
 * workspace.  RGCN_ERR_UNSUPPORTED: k > 64, num_nodes >= 2^31.  num_queries == 0: RGCN_OK before any pointer is
 * looked at. */
int rgcn_paths_topk(const int64_t* out_ptr, const int32_t* out_dst, const float* edge_score,
                    const int64_t* in_ptr, const int32_t* in_src, const int64_t* in_pos,
                    int64_t num_nodes, int64_t nnz,
                    const int64_t* sources, const int64_t* targets, int64_t num_queries,
                    int max_len, int k, int slices,
                    int32_t* nodes, int32_t* length, float* score,
                    int64_t* count, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_PATHS_H */
