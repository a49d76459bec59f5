/* rgcn_softmax.h - the 1-vs-all softmax loss over every candidate of librgcn_hip.so (plain C, gfx950 only).
 *
 * The error codes, the ABI version, the alignment rule and the conventions (device pointers, `stream` a hipStream_t
 * passed as void*, asynchronous, no allocation, no host synchronisation, nothing aborts) are those of rgcn_hip.h.  The
 * candidate masks are the ranking pass's (distmult_rank_masked, distmult_topk_masked): W = ceil(N / 32) words per row,
 * entity n is bit (n & 31) of word (n >> 5); `allow` is uint32[classes, W] read through query_class int32[batch],
 * `exclude` is uint32[batch, W]; either may be NULL ("allows everything" / "strikes nothing").
 *
 * For query rows q [B, d], candidate rows E [N, d] and target int64[B], with this grouping (the grouping is part of
 * the contract):
 *
 *   s[b, n]     = <q[b], E[n]>     the k-ordered fp32 MFMA chain of the shared tile (csrc/rgcn_mma_f32_dma.h): the bits
 *                                  distmult_score_all_tails stores and the ranking and top-k passes compare
 *   eligible(b) = { n : allow[query_class[b]] admits n and exclude[b] does not strike it }  U  { target[b] }
 *   m[b]        = max over eligible n of s[b, n]
 *   lse[b]      = m[b] + log( sum over eligible n of exp(s[b, n] - m[b]) )
 *   loss[b]     = lse[b] - s[b, target[b]]
 *   hit[b]      = s[b, target[b]] >= m[b]
 *
 * The target is ALWAYS eligible: when its own exclude bit is set (in training it always is: the positive is a known
 * triple), when its class is not the allowed one, when the query's class allows nothing.  A query class outside
 * [0, classes) leaves only the target eligible, as in the top-k pass.  s[b, target[b]] is taken from the accumulator of
 * the tile that holds the target: the term inside the sum and the term subtracted from it are the same bits.
 *
 * Gradients, for g[b] = d (whatever follows) / d loss[b] (the mean is the caller's reduction, as with BCE):
 *
 *   c[b, n]  = g[b] * ( [n eligible] exp(s[b, n] - lse[b]) - [n == target[b]] )
 *   dq[b, :] = sum_n c[b, n] E[n, :]
 *   dE[n, :] = sum_b c[b, n] q[b, :]
 *
 * There is no scatter for the target: it is the second term of the coefficient.  The whole [N, d] gradient is written
 * by the call (rows no query finds eligible as exact zeros); the caller does not clear it.
 *
 * Order of every sum (no floating-point atomics; two calls with the same arguments give the same bits):
 *   - The candidates are cut into 128-column tiles, the tiles into S contiguous slices of ceil(tiles / S) tiles (the
 *     last one shorter, none empty).  slices > 0: S = min(slices, tiles, 64).  slices == 0: S is chosen from B and N
 *     alone - 1 when ceil(B / 64) >= 128, else min(ceil(256 / ceil(B / 64)), tiles, 64).  The result may depend on S
 *     in the last bits.
 *   - Forward: inside a slice, a (row, column mod 32, column-group pair) chain keeps a running (m, sum) over its
 *     tiles in ascending order, the sum rescaled by exp(m_old - m_new) when the maximum moves; the 32 chains of a row
 *     are merged by a butterfly (lane distance 1, 2, 4, 8, 16), then the two column-group pairs, then the slices in
 *     slice order - that last merge and lse = m + log(sum) in float64, lse rounded to fp32 once (a 1-ulp logf errs to
 *     the same side for every row of an untrained model, and the rows' coefficient sums then add up in the encoder's
 *     gradients).  A merge of (m1, l1) and (m2, l2) is m = max, l = l1 exp(m1 - m) + l2 exp(m2 - m), the factor of
 *     the side that holds the maximum being exactly 1; -inf maxima never meet in a subtraction.
 *   - dq: per slice, candidate tiles ascending, inside a tile the second product's k order (8-candidate steps, the
 *     MFMA chain of the shared tile); the S partial slabs are added in slice order.
 *   - dE: a workgroup owns 64 candidate rows and walks ALL queries in ascending 128-query tiles: no slices.
 *     accumulate != 0 starts from what dE holds instead of zero (a caller that feeds the batch in chunks, in chunk
 *     order: dE = (chunk 0) + (chunk 1) + ...).
 *
 * Forward-error bounds (tests/softmax_reference.py computes them from the data), u = 2^-24:
 *   |s - s64|     <= gamma_d * sum_k |q_k| |E_nk|,  gamma_d = d u / (1 - d u)
 *   |lse - lse64| <= max_n |s - s64| + (5 T + 2 + ln N) u + u |lse64|, T = the float32 merge steps on the longest
 *                    chain (tiles of a slice + 5 + 1): log-sum-exp is 1-Lipschitz in the sup norm, all summands are
 *                    positive; every step adds at most five roundings to the sum's relative error (the factor's expf
 *                    at 1 ulp = 2 u, its product, the pair's sum, the step's sum); the rounding of s - m moves a term
 *                    by |s - m| u relatively, which weighted by the terms themselves is at most (ln N) u; the slice
 *                    merge and the logarithm run in float64 (their roundings are inside the 2 u) and m + log(sum)
 *                    is rounded to fp32 once.
 *   the coefficient and gradient bounds follow from the same two quantities (tests/softmax_reference.py).
 *
 * Non-finite values: plain fp32 arithmetic in the grouping above.  An eligible -inf score contributes an exact zero;
 * an eligible NaN or +inf makes that row's lse, loss and coefficients what the same grouping gives in float64 (NaN);
 * rows are independent in lse, loss, hit and dq; an ineligible candidate's score never matters and its coefficient is
 * an exact 0 (selected, not multiplied); dE rows inherit non-finite coefficients as the restatement does.
 * The two products of the backward are matrix products, in the restatement too: a 0 coefficient against a NaN or
 * infinite row of E or q is 0 * NaN there as here.
 *
 * Arguments: d a multiple of 32 (RGCN_ERR_UNSUPPORTED otherwise; d <= 0 is RGCN_ERR_ARG) and at most 256
 * (RGCN_ERR_UNSUPPORTED).  batch == 0 with valid sizes is RGCN_OK before any pointer is looked at (the backward still
 * writes dE as zeros when it is given and accumulate is 0).  A target outside [0, N) is clamped to 0 and raises the
 * sticky flag (rgcn_index_error_fetch).  Pointers: q, emb, dq, dE and the workspace at 16 bytes, target at
 * 8, masks and per-row vectors at 4 (RGCN_ERR_ALIGN, checked last).  The first call on a device looks up the address
 * of the sticky flag, which is not a stream operation.  Not forwarded by rgcn_sequence_run.
 */
#ifndef RGCN_SOFTMAX_H
#define RGCN_SOFTMAX_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace either entry point needs for this shape and `slices` (0 for an empty batch or invalid sizes). */
size_t rgcn_softmax_workspace_bytes(int64_t batch, int64_t num_entities, int64_t d, int64_t slices);

/* Forward.  lse, true_score, row_max: float[batch], required.  loss float[batch] and hit int32[batch]: optional
 * (NULL: not written), formed by the launch that merges the slices.
 * RGCN_ERR_WORKSPACE: workspace NULL or smaller than rgcn_softmax_workspace_bytes says. */
int rgcn_softmax_lse(const float* q, const float* emb, const int64_t* target, const uint32_t* allow,
                     const int32_t* query_class, int64_t num_classes, const uint32_t* exclude, int64_t batch,
                     int64_t num_entities, int64_t d, int64_t slices, float* lse, float* true_score, float* row_max,
                     float* loss, int32_t* hit, void* workspace, size_t workspace_bytes, void* stream);

/* Backward.  g, lse: float[batch].  dq float[batch, d], dE float[num_entities, d]: a NULL one is not computed.
 * accumulate: see "Order of every sum" (dE only; dq is always written). */
int rgcn_softmax_grad(const float* g, const float* q, const float* emb, const int64_t* target, const uint32_t* allow,
                      const int32_t* query_class, int64_t num_classes, const uint32_t* exclude, const float* lse,
                      int64_t batch, int64_t num_entities, int64_t d, int64_t slices, float* dq, float* dE,
                      int accumulate, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_SOFTMAX_H */
