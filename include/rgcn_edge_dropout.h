/* rgcn_edge_dropout.h - edge dropout and hidden batch edges for the training encoder of librgcn_hip.so (plain C,
 * gfx950 only).
 *
 * The error codes, the ABI version and the conventions (device pointers, `stream` a hipStream_t passed as void*,
 * nothing aborts, inputs never written) are those of rgcn_hip.h.
 *
 * Why.  A link-prediction trainer that encodes over the train graph and scores positives taken from that same graph
 * asks the model to predict an edge the encoder has just averaged into both of its endpoints.  Schlichtkrull et al.
 * (2018) name edge dropout as the regulariser that makes the R-GCN encoder work for this task, and later trainers
 * also take the batch's own edges out of the message-passing graph.  The reference has neither.  The bucketed
 * structure is built once by a sort that synchronises and allocates, so it cannot change per step; what can change
 * per step is the per-edge weight the weighted gathers already multiply by.  Hence: a VIEW of a graph handle whose
 * two directions are both weighted, and a DRAW that rewrites the view's weights in place.
 *
 * THE VIEW.  rgcn_edge_dropout_create takes a square handle with a mean forward direction (what rgcn_graph_create and
 * rgcn_graph_import return; anything else: RGCN_ERR_UNSUPPORTED) and builds an rgcn_graph whose two directions are
 * weighted-sum structures.  The view SHARES rowptr, col, perm, the work items, the hub index, the item heads' column
 * ids and the occupancy masks with the parent - it does not own them, and the parent must outlive the view.  The
 * view OWNS, per direction, val (float[E]) and head_w (float[level-0 items * 8]), one int32[N * R] array of kept
 * counts (and the int32[N * R] counters a draw adds into, and two float[N * R] arrays: M of a mask or attention draw, mx of
 * an attention draw), and two int32[E] index arrays (the forward segment of
 * every forward position and of every transposed position), which make the draw a flat walk of the edges, and twin
 * (int32[E], below).  Ownership lives in the wrapper, not in the structure:
 * rgcn_edge_dropout_destroy frees only what the view owns.  After create the view holds the draw p = 0,
 * position = NULL, so it is usable at once.  create may allocate and synchronise; what it allocates besides the view's
 * own arrays (the sorts that pair the twins) is freed before it returns.
 *
 * TWINS - the contract; tests restate it on the host (tests/edge_dropout_twins_reference.py).  Data that stores a pair as
 * two columns, (h, r, t) and (t, r, h), has to hide and drop them together.  twin is indexed by ORIGINAL column.  For a
 * triple (a, r, b) with a != b let F be the columns holding (src, rel, dst) = (a, r, b) in ascending order and B the
 * columns holding (b, r, a) in ascending order: twin[F[j]] = B[j] and twin[B[j]] = F[j] for j < min(|F|, |B|).  Every
 * other column has twin = -1: a column whose reversed triple is not stored, a self loop, and the SURPLUS copies of the
 * longer side (the last |F| - |B| of F or |B| - |F| of B) - as a duplicate column of a batch triple that is not itself
 * in the window is not hidden either.  The relation must be equal: (a, 0, b) and (b, 1, a) are not twins.  twin is an
 * involution on the columns that have one.  Built on the device (two stable radix sorts and one pairing kernel) for
 * every graph create accepts; 4 bytes per edge stay resident.
 *
 * Every entry point that takes an rgcn_graph takes rgcn_edge_dropout_graph(ed):
 *   rgcn_aggregate(view, 0, x)   agg[i * R + r] = sum over the in-edges of (i, r) of w_fwd * x[src], in the weighted
 *                                gather's order (runs, packs and the hub tree included) = the mean over the KEPT
 *                                in-edges up to rounding; a segment without a kept edge gives zeros.  This is RGCNConv
 *                                on edge_index[:, kept], edge_type[kept].
 *   rgcn_aggregate(view, 1, g)   its adjoint.
 *   rgcn_graph_weight_bound      a true bound for EVERY draw: forward 1 + 1e-6 (a segment's weights sum to
 *                                k * fl(1 / k) <= 1 + 2^-23), transposed the edge count of the longest (source,
 *                                relation) segment (every weight is <= 1).  A mask draw (below) with values in
 *                                [0, inf) keeps both: transposed because every weight is still <= 1 (a rounded sum
 *                                of non-negative terms is never below one of them - rounding is monotone - so
 *                                M >= m and fl(m / M) <= 1), forward because M is a sum of non-negative terms through at most h rounded
 *                                additions on any path of its fixed order - h = ceil(L / 8) + 3 for a segment of
 *                                L <= 64 edges, ceil(L / 256) + 6 + 3 past that - so M >= (sum m) (1 - u)^h, u = 2^-24,
 *                                each quotient is <= (m / M) (1 + u), and the weights of a segment sum to at most
 *                                (1 + u) / (1 - u)^h.  Up to L = 1,280 that is below the float 1 + 1e-6 rounds to
 *                                (1 + 16 u) and the value is what it always was; a view whose longest forward segment
 *                                is longer returns (1 + u) / (1 - u)^h rounded up, e.g. 1 + 7.9e-6 at 31,017 edges.
 *                                Negative or non-finite mask values void the bound.
 *   tile / row occupancy masks   the parent's: supersets under every draw (a tile they skip is zero under every draw).
 *
 * THE DRAW - the contract; tests restate it on the host (tests/edge_dropout_reference.py).  With e the ORIGINAL
 * column of an edge (perm[] of either direction), c0 = cursor[0] (0 without a cursor), seed = rng[0], epoch = rng[1]:
 *   hidden(e)  = position != NULL  and  c0 <= position[e] < c0 + batch
 *   c          = philox4x32_10(counter = (low32(e), low32(c0), low32(epoch), RGCN_EDGE_DROPOUT_STREAM),
 *                              key = (low32(seed), high32(seed)))
 *   dropped(e) = c[0] < T,   T = floor(p * 2^32) as uint32            - an integer compare: the host restates it exactly
 *   kept(e)    = not hidden(e) and not dropped(e)
 *   k[i, r]    = number of kept edges of forward segment (i, r)      - int32, exact (integer atomics: order-free)
 *   w_fwd[pos] = kept ? 1.0f / (float)k[dst, r] : 0.0f               - one IEEE division, as the transposed weights of
 *   w_t[pos]   = kept ? 1.0f / (float)k[dst, r] : 0.0f                 rgcn_graph_create (dst = col_t[pos], r = segment % R)
 *   head_w     = the copies of the first weights of every level-0 item, refreshed for both directions
 *   stats[0]  += kept edges,  stats[1] += hidden edges               - accumulated, never cleared here
 * p = 0 without a position reproduces the parent's transposed weights bit for bit.  The word depends on (seed, epoch,
 * cursor, column) only: the same step draws the same mask whatever ran before it, and a replayed HIP graph whose device
 * cursor has moved draws that cursor's mask.
 * The two option bits of `batch` (below) change two lines of the above and nothing else; `batch` above is the window's
 * LENGTH, batch with both bits cleared.  With in_window(x) = c0 <= position[x] < c0 + length:
 *   RGCN_EDGE_DROPOUT_HIDE_TWINS  hidden(e) = position != NULL and (in_window(e) or (twin[e] >= 0 and in_window(twin[e])))
 *   RGCN_EDGE_DROPOUT_PAIRED      counter word 0 of the Philox call is low32(twin[e] >= 0 ? min(e, twin[e]) : e): a pair
 *                                 shares one word and is dropped or kept together
 * stats[1] counts every hidden edge once, twins included.  k, both val, both head_w, the three launches without a memset
 * node, capture and the absence of any allocation are as above.  A draw with an option reads twin[e] and, for
 * HIDE_TWINS, position[twin[e]] on top of what the plain draw reads; the plain draw reads neither.
 *
 * THE MASK DRAW - RGCN_EDGE_DROPOUT_MASK, a third option bit of `batch`; tests restate it on the host
 * (tests/edge_mask_reference.py).  With the bit set the call draws nothing and its parameters take these roles:
 *   p          must be 0 (RGCN_ERR_ARG otherwise); RGCN_EDGE_DROPOUT_PAIRED has no word to share: RGCN_ERR_ARG.
 *   rng        NOT {seed, epoch}: DEVICE const float mask[E], indexed by ORIGINAL column, read and never written.  It
 *              still needs 8 bytes (RGCN_ERR_ALIGN) and must not be NULL.
 *   cursor, position, batch's length, RGCN_EDGE_DROPOUT_HIDE_TWINS, stats      as in the plain draw: hard hiding
 *              composes with the soft mask.
 * With e the original column of a position and s = (dst, r) its forward segment:
 *   m(e)      = hidden(e) ? 0.0f : mask[e]          a select: a hidden column's value is never looked at.  Nothing is
 *               clamped - plain fp32 arithmetic: a NEGATIVE value enters M as it is and gives a negative weight where
 *               M > 0; a NaN makes M NaN, and M > 0 is then false: every weight of that segment is 0.  Neither is
 *               counted in k.  Denormal values are summed and divided as the denormals they are.
 *   M[s]      = the sum of m over the positions of s in this FIXED order - the one rgcn_hip.h states for S[s] under
 *               RGCN_MODE_MEAN_GRAD - b the segment's first position, every partial sum starting from +0.0f:
 *                 <= 64 edges  eight partial sums P_j = m[b + j] + m[b + j + 8] + m[b + j + 16] + ... (in that order),
 *                              M = ((P_0 + P_4) + (P_2 + P_6)) + ((P_1 + P_5) + (P_3 + P_7));
 *                  > 64 edges  256 partial sums T_t = m[b + t] + m[b + t + 256] + ... (in that order); each 64
 *                              consecutive ones are combined by an xor butterfly with the offsets 32, 16, 8, 4, 2, 1
 *                              (entry l becomes entry l + entry (l ^ offset) at every step) into W_v, and
 *                              M = ((W_0 + W_1) + W_2) + W_3.  A hub segment of any length takes this rule.
 *               No floating-point atomics: two calls with the same arguments leave the same bits.
 *   w_fwd[pos] = w_t[pos'] = M[s] > 0 ? m(e) / M[s] : 0.0f          one IEEE division; the same value in both directions
 *   head_w     refreshed for both directions, as the plain draw does
 *   k[s]       = the number of positions of s with m(e) > 0 (int32)  - rgcn_edge_dropout_kept
 *   stats[0]  += edges with m(e) > 0,  stats[1] += hidden edges
 * mask = 1 everywhere is the draw p = 0 bit for bit (a sum of n < 2^24 ones is exact in every order), and a mask of
 * zeros and ones is the plain draw p = 0 with exactly the zero columns hidden through `position`.  Three kernels, no
 * memset node, no allocation (M lives in a float[N * R] create allocated), no host synchronisation: capturable.  The
 * plain draw's launches are not the mask draw's and run the instructions they always ran.
 *
 * THE ATTENTION DRAW - RGCN_EDGE_DROPOUT_ATTENTION, a fourth option bit of `batch`; tests restate it on the host
 * (tests/attention_reference.py).  A segment's weights are the softmax of per-edge logits formed from per-(node,
 * relation) scalars: within-relation attention on the layer's input (Busbridge et al. 2019).  Nothing is drawn and the
 * parameters take these roles:
 *   p          the negative slope of the leaky ReLU, 0 <= p <= 1 (anything else, NaN included: RGCN_ERR_ARG); the
 *              kernels use (float)p.  RGCN_EDGE_DROPOUT_MASK or RGCN_EDGE_DROPOUT_PAIRED beside the bit: RGCN_ERR_ARG.
 *              Nothing is launched on a refusal.
 *   rng        NOT {seed, epoch}: DEVICE const float a[2 * N * R], read and never written: a[i * R + r] = a_dst[i, r],
 *              a[N * R + j * R + r] = a_src[j, r].  It needs 8 bytes (RGCN_ERR_ALIGN) and must not be NULL.
 *   cursor, position, batch's length, RGCN_EDGE_DROPOUT_HIDE_TWINS, stats      as in the plain draw: hard hiding
 *              composes with attention.
 * With e = (j -> i, r) the edge of a position and s = (i, r) its forward segment:
 *   z(e)      = a[i * R + r] + a[N * R + j * R + r]                one fp32 addition
 *   l(e)      = z(e) >= 0 ? z(e) : fl((float)p * z(e))             a select; the product rounded by itself
 *   mx[s]     = the maximum of l over the positions of s that are not hidden (a NaN is passed over; -inf without one)
 *   m(e)      = hidden(e) ? 0.0f : exp(fl(l(e) - mx[s]))           a select: a hidden edge's scalars change nothing.
 *               exp is expf of the ROCm device library, fp32 in and out, without fast-math: the contract is an error of
 *               at most 2 ulp (the library's table says 1), exp(+-0) = 1 exactly, exp(-inf) = +0, results below the
 *               normal range may be flushed or denormal, and the same argument gives the same bits on every call.
 *   M[s]      = the sum of m over the positions of s in the FIXED order stated above for the mask draw
 *   k[s]      = the number of positions of s that are not hidden (int32)  - rgcn_edge_dropout_kept
 *   w_fwd[pos] = w_t[pos'] = k[s] > 0 ? m(e) / M[s] : 0.0f          one IEEE division; the same value in both directions
 *   head_w     refreshed for both directions
 *   stats[0]  += edges that are not hidden,  stats[1] += hidden edges
 * The maximum contributes exp(0) = 1, so M[s] >= 1 for finite logits and no quotient overflows.  a = 0 everywhere is
 * the plain draw p = 0 under the same hiding, bit for bit: every m is 1, a sum of fewer than 2^24 ones is exact in any
 * order, and the division is the same.
 * Non-finite values: a NaN logit (exp of it is NaN) or a +inf one (inf - inf) makes M[s] NaN and with it EVERY weight
 * of that segment, hidden positions included (0 / NaN) - the layer's output raises the alarm; so does
 * a segment whose non-hidden logits are all -inf.  A -inf logit beside a finite one has weight +0.  No other segment
 * is touched, and a segment whose edges are all hidden holds zeros (k = 0) whatever its scalars are.
 * Three kernels, no memset node, no allocation (mx and M live in two float[N * R] arrays create allocated), no host
 * synchronisation: capturable.  The plain draw's and the mask draw's launches are not this draw's and run the
 * instructions they always ran.  rgcn_graph_weight_bound of the view stays true: the weights are non-negative and
 * normalised by the mask draw's rule - a quotient by a sum in the same fixed order - so the mask draw's argument above
 * carries over word for word with m = exp(l - mx) in [0, 1] (while the logits are finite; a NaN voids it as there).
 *
 * Non-finite values - a deliberate deviation.  A dropped or hidden edge contributes 0 * x: it is MULTIPLIED by a zero
 * weight, not skipped, so a non-finite source row still reaches the aggregate of a segment it was dropped from
 * (0 * NaN = NaN), where RGCNConv on the kept subgraph would not see it.  The hot gather is not changed for it.
 */
#ifndef RGCN_EDGE_DROPOUT_H
#define RGCN_EDGE_DROPOUT_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGCN_EDGE_DROPOUT_STREAM 0x45444F50u   /* counter word 3 of every edge-dropout draw ("EDOP"; not RGCN_RESAMPLE_STREAM) */

/* Option bits of rgcn_edge_dropout_draw's `batch` (as RGCN_MODE_SPARSE_ROWS rides in a mode word): the window's length
 * is `batch` with all of them cleared, and a draw with none set writes the bytes it always wrote. */
#define RGCN_EDGE_DROPOUT_HIDE_TWINS (1LL << 62)   /* a column whose twin stands in the window is hidden too */
#define RGCN_EDGE_DROPOUT_PAIRED     (1LL << 61)   /* a column and its twin share one Philox word: dropped or kept together */
#define RGCN_EDGE_DROPOUT_MASK       ((int64_t)1 << 60)   /* = 1LL << 60.  THE MASK DRAW above: rng is const float mask[E], p must be 0 */
#define RGCN_EDGE_DROPOUT_ATTENTION  ((int64_t)1 << 59)   /* = 1LL << 59.  THE ATTENTION DRAW above: rng is const float a[2 * N * R], p the slope */

typedef struct rgcn_edge_dropout rgcn_edge_dropout;

/* RGCN_ERR_ARG: g or out NULL.  RGCN_ERR_UNSUPPORTED: g is not a square handle with a mean forward direction and a
 * weighted transposed one (a shard, another view).  Synchronises `stream` and allocates device memory owned by the view. */
int rgcn_edge_dropout_create(const rgcn_graph* g, void* stream, rgcn_edge_dropout** out);
void rgcn_edge_dropout_destroy(rgcn_edge_dropout* ed);
/* the view; owned by ed, valid until rgcn_edge_dropout_destroy */
const rgcn_graph* rgcn_edge_dropout_graph(const rgcn_edge_dropout* ed);
/* DEVICE int32[N * R]: k of the last draw; owned by ed */
const int32_t* rgcn_edge_dropout_kept(const rgcn_edge_dropout* ed);
/* the same array copied (device to device, async on `stream`) into the caller's int32[N * R], as rgcn_graph_export
 * copies the structure's arrays.  RGCN_ERR_ARG: ed NULL, or out NULL while N * R > 0; RGCN_ERR_ALIGN: out needs 4. */
int rgcn_edge_dropout_kept_export(const rgcn_edge_dropout* ed, int32_t* out, void* stream);

/* One draw: asynchronous on `stream`, no allocation, no host synchronisation, capturable into a HIP graph (three
 * kernels, no memset node: the draw's last launch clears the counters the next one adds into).  rng: DEVICE int64[2] =
 * {seed, epoch}; cursor: DEVICE int64[1] or NULL (= 0); batch >= 0: the window's length, below 2^59, ORed with any of
 * RGCN_EDGE_DROPOUT_HIDE_TWINS and RGCN_EDGE_DROPOUT_PAIRED, or with RGCN_EDGE_DROPOUT_MASK (rng is the mask then), or
 * with RGCN_EDGE_DROPOUT_ATTENTION (rng holds the attention scalars, p the slope in [0, 1]);
 * position: DEVICE int64[E] or NULL, position[e] = where column e stands in the epoch's order; stats: DEVICE int64[2]
 * or NULL.  RGCN_ERR_ARG: ed or rng NULL, batch < 0, p outside [0, 1) (NaN included).  RGCN_ERR_ALIGN: rng, cursor,
 * position, stats need 8.  With RGCN_EDGE_DROPOUT_MASK: p != 0 or RGCN_EDGE_DROPOUT_PAIRED RGCN_ERR_ARG (after the range
 * of p, before the alignment).  With RGCN_EDGE_DROPOUT_ATTENTION: p outside [0, 1], RGCN_EDGE_DROPOUT_MASK or
 * RGCN_EDGE_DROPOUT_PAIRED RGCN_ERR_ARG, then the alignment. */
int rgcn_edge_dropout_draw(rgcn_edge_dropout* ed, double p, const int64_t* rng, const int64_t* cursor, int64_t batch,
                           const int64_t* position, int64_t* stats, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_EDGE_DROPOUT_H */
