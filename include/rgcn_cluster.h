/* rgcn_cluster.h - k-means and silhouette analysis of embedding rows of librgcn_hip.so (plain C, gfx950 only).
 *
 * The error codes, the ABI version and the conventions (device pointers, `stream` a hipStream_t passed
 * as void*, asynchronous, no allocation, nothing aborts) are those of rgcn_hip.h.
 *
 * Common to every call: x float32[M, d] contiguous, d % 32 == 0 (else RGCN_ERR_UNSUPPORTED), 2 <= M < 2^30,
 * 2 <= k <= RGCN_CLUSTER_MAX_K (k above the cap: RGCN_ERR_UNSUPPORTED; M < 2, k < 2, d <= 0: RGCN_ERR_ARG).
 * The k-means calls take R restarts at once, 1 <= R <= RGCN_CLUSTER_MAX_RESTARTS: centroids float32[R, k, d],
 * labels int32[R, M], done int32[R] (device flags, may be NULL = no restart is done).  A restart whose done flag is
 * non-zero is FROZEN: no call below writes any of its outputs.  Every sum is formed in an order fixed by
 * (M, d, k, R) alone and there are no floating-point atomics: the same inputs give the same bits on every call.
 */
#ifndef RGCN_CLUSTER_H
#define RGCN_CLUSTER_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGCN_CLUSTER_MAX_K 64
#define RGCN_CLUSTER_MAX_RESTARTS 1024

/* Bytes of workspace the three k-means calls need (one size serves all three); 0 for arguments they refuse. */
size_t rgcn_kmeans_workspace_bytes(int64_t M, int64_t d, int64_t R, int64_t k);

/* Assignment of every row to its nearest centroid, all restarts in one launch of the fp32 matrix-core tile
 * (B operand: the R * ceil32(k) centroid rows, every restart padded to a multiple of 32 columns).
 *   key(i, c)  = |c|^2 - 2 <x_i, c>   in fp32 (|x_i|^2 does not change the arg-min and is left out)
 *   labels[r, i] = the c in [0, k) of least key.  Equal keys go to the LOWER cluster id.  A NaN key never wins
 *                  against a key that is not NaN (+inf included); a row whose keys are all NaN gets the lowest id.
 *   num_changed[r] (int32) = the number of rows i with labels[r, i] != labels_prev[r, i].
 * labels_prev may be the same array as labels (an entry is read before it is written) or NULL (every row counts
 * as changed).  Pad columns carry key +inf and are never chosen.
 * RGCN_ERR_ARG also for: R < 1, a NULL x / centroids / labels / num_changed, a NULL or short workspace.
 * RGCN_ERR_UNSUPPORTED also for R above the cap. */
int rgcn_kmeans_assign(const float* x, int64_t M, int64_t d, const float* centroids, int64_t R, int64_t k,
                       const int32_t* labels_prev, int32_t* labels, int32_t* num_changed, const int32_t* done,
                       void* ws, size_t ws_bytes, void* stream);

/* Update: for every (restart, cluster) the member count and the mean of the member rows, written over the centroid.
 *   counts int32[R, k]; a cluster WITHOUT members keeps its previous centroid and has count 0.  (scikit-learn moves
 *   an empty cluster to the row farthest from its centre; this library does not relocate.)
 *   shift2 float32[R] = sum over c of |c_new - c_old|^2.
 *   num_iter int32[R] is incremented for every restart that is not done.
 *   done[r] is SET when num_changed[r] == 0 (no label changed in this iteration's assignment) or
 *   shift2[r] <= tol_abs.  Once set, the restart is frozen, so the host may look at the flags at any interval
 *   without changing a result bit.  done may be NULL: nothing is frozen and nothing is set.
 * Labels must be in [0, k) (rgcn_kmeans_assign's are).
 * RGCN_ERR_ARG also for: R < 1, tol_abs < 0 or NaN, a NULL x / centroids / labels / num_changed / counts / shift2 /
 * num_iter, a NULL or short workspace. */
int rgcn_kmeans_update(const float* x, int64_t M, int64_t d, float* centroids, int64_t R, int64_t k,
                       const int32_t* labels, const int32_t* num_changed, int32_t* counts, float* shift2,
                       int32_t* num_iter, int32_t* done, float tol_abs, void* ws, size_t ws_bytes, void* stream);

/* inertia double[R] = sum over i of |x_i - c_labels[r, i]|^2, from the rows themselves (not from the keys, whose
 * cancellation it avoids): fp32 differences and squares summed per row in fp32, the rows in double.  Done flags
 * do not apply: every restart is computed. */
int rgcn_kmeans_inertia(const float* x, int64_t M, int64_t d, const float* centroids, int64_t R, int64_t k,
                        const int32_t* labels, double* inertia, void* ws, size_t ws_bytes, void* stream);

/* Silhouette samples.  The caller hands over the rows twice: x in its own order, and xs float32[Mp, d], the same
 * rows grouped by label, every label's segment padded to a multiple of 32 rows, Mp a multiple of 128:
 *   col_row     int32[Mp]       the row of x that sits in row n of xs, -1 for a pad row (pad rows may hold anything
 *                               finite; they contribute 0)
 *   blk_cluster int32[Mp / 32]  the label of every 32-row block of xs, ascending, -1 for a block of pad rows only
 *   counts      int32[k]        members per label (0: a label nobody carries - skipped, not "distance 0")
 *   labels      int32[M]        in [0, k)
 * With dist(i, j) = sqrt(max(0, |x_i|^2 + |x_j|^2 - 2 <x_i, x_j>)) in fp32, dist(i, i) exactly 0, and
 * S[i][c] = sum of dist(i, j) over the members j of c:
 *   a = S[i][own] / (n_own - 1),  b = min over the non-empty other labels of S[i][c] / n_c,
 *   s[i] = (b - a) / max(a, b);   s[i] = 0 where n_own == 1, where max(a, b) == 0 and where no other label has a member.
 * The Gram trick cancels less the nearer the rows are to the origin: hand over rows centred at their mean
 * (distances do not change).  slices: workgroups that share one 64-row tile (they divide the columns); 0: chosen
 * from M (about four workgroups per compute unit); at most 256 are used.  For a given slices the output is the
 * same bits on every call; across slice counts it agrees to rounding.
 * s float32[M] in the order of x; mean double[1] = the mean of s, summed in a fixed order in double.
 * RGCN_ERR_ARG also for: Mp < M, Mp % 128 != 0, slices < 0, a NULL array, a NULL or short workspace. */
size_t rgcn_silhouette_workspace_bytes(int64_t M, int64_t Mp, int64_t k, int64_t slices);
int rgcn_silhouette_samples(const float* x, const float* xs, const int32_t* col_row, const int32_t* blk_cluster,
                            const int32_t* counts, const int32_t* labels, int64_t M, int64_t Mp, int64_t d, int64_t k,
                            int64_t slices, float* s, double* mean, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_CLUSTER_H */
