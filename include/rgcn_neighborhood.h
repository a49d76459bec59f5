/* rgcn_neighborhood.h - local-neighbourhood statistics of node pairs of librgcn_hip.so (plain C, gfx950 only).
 *
 * The error codes, the ABI version and the conventions (device pointers, `stream` a hipStream_t passed
 * as void*, asynchronous, no allocation, nothing aborts) are those of rgcn_hip.h.
 */
#ifndef RGCN_NEIGHBORHOOD_H
#define RGCN_NEIGHBORHOOD_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGCN_NEIGHBORHOOD_MAX_RADIUS 4
#define RGCN_NEIGHBORHOOD_MAX_CLASSES 32
#define RGCN_NEIGHBORHOOD_MAX_COMMON 1024
/* An adjacency row of at least this many entries is walked by a whole wave, 64 entries at a time; a shorter one by the
 * lane that found it.  Nothing in the results depends on it. */
#define RGCN_NEIGHBORHOOD_HUB_DEGREE 64

/* The structure is the one rgcn_paths.h describes, the node-level digraph as two CSRs over the UNIQUE (src, dst) pairs
 * (nnz of them; in_pos is not needed here):
 *   out_ptr int64[num_nodes + 1], out_dst int32[nnz]   the pairs by src, then dst ascending
 *   in_ptr  int64[num_nodes + 1], in_src  int32[nnz]   the same pairs by dst, then src ascending
 * Self loops may be present. */

/* The largest num_nodes rgcn_pair_neighborhood takes: a workgroup keeps four bitsets over the nodes in its LDS.  At
 * least 262,144. */
int64_t rgcn_neighborhood_max_nodes(void);

/* The radius-`radius` balls around sources[q] and targets[q], their intersection and their union, for num_queries
 * queries.
 *
 * Contract:
 *   - nbr(u) = out(u) + in(u): successors and predecessors.  A node is PRESENT when it has at least one out- or
 *     in-entry (a self loop counts).
 *   - B_0(x) = {x} when x is present, else empty; B_j(x) = B_{j-1}(x) + nbr(B_{j-1}(x)).  An absent x, or one outside
 *     [0, num_nodes), has empty balls at every radius; nothing is read for an id outside the range.
 *   - radius in 0..4; sources[q] == targets[q] is an ordinary query.  With r = radius:
 *   - ball int64[Q, 2, 5]: ball[q, side, j] = |B_j(x)| for j <= r and 0 for j > r; side 0 is the source, side 1 the
 *     target.  (ball[.., 1] - 1 of a present x: its distinct neighbours, x itself not counted even with a self loop.)
 *   - distance int32[Q]: the smallest j <= r with targets[q] in B_j(sources[q]), else -1: the undirected hop distance
 *     when it is at most r.
 *   - common int64[Q] = |B_r(s) & B_r(t)|; union_nodes int64[Q] = |B_r(s) + B_r(t)|.
 *   - union_edges int64[Q]: the out-entries (u, v) with both ends in the union - every unique directed pair once, self
 *     loops included.
 *   - class_count int64[Q, num_classes]: the union's nodes per class, node_class int32[num_nodes]; a node whose class
 *     is negative or >= num_classes is counted nowhere.  num_classes in 0..32.  Written only when node_class is not
 *     NULL and num_classes > 0.
 *   - common_nodes int32[Q, common_cap]: the common_cap smallest ids of the intersection, ascending, -1 past them.
 *     common_cap in 0..1024.  Written only when common_cap > 0.
 *   - Every output of every query is written, zeros and -1 padding included.  Every sum is an integer sum: the result
 *     does not depend on how the waves are scheduled.
 *   - There is no workspace.
 *
 * RGCN_ERR_ARG: num_queries < 0, num_nodes <= 0, nnz < 0, radius outside 0..4, num_classes outside 0..32, common_cap
 * outside 0..1024; with num_queries > 0: a NULL array (out_dst / in_src may be NULL when nnz == 0; class_count and
 * common_nodes when they are not written; node_class always).  RGCN_ERR_UNSUPPORTED: num_nodes >
 * rgcn_neighborhood_max_nodes().  num_queries == 0: RGCN_OK before any pointer is looked at. */
int rgcn_pair_neighborhood(const int64_t* out_ptr, const int32_t* out_dst, const int64_t* in_ptr, const int32_t* in_src,
                           int64_t num_nodes, int64_t nnz,
                           const int64_t* sources, const int64_t* targets, int64_t num_queries, int radius,
                           const int32_t* node_class, int num_classes, int common_cap,
                           int64_t* ball, int32_t* distance, int64_t* common, int64_t* union_nodes, int64_t* union_edges,
                           int64_t* class_count, int32_t* common_nodes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_NEIGHBORHOOD_H */
