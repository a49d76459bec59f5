/* rgcn_resample.h - bootstrap resampling of the evaluation metrics of librgcn_hip.so (plain C, gfx950 only).
 *
 * The error codes, the ABI version and the conventions (device pointers, `stream` a hipStream_t passed as void*,
 * asynchronous, no allocation, nothing aborts, inputs never written) are those of rgcn_hip.h.
 *
 * Answers the reference's `statistical_significance_test` (src/compare_methods.py:701-740), which writes
 * exp(-10 |difference|) into a table and notes "would need multiple runs or bootstrap": the sufficient statistics of
 * AUC-ROC, average precision, the threshold metrics and the ranking metrics under `replicates` paired resamples of the
 * test triples, from one walk of the sorted scores (or of the ranks) per four replicates.
 *
 * THE RESAMPLING RULE - the contract; tests restate it on the host (tests/resample_reference.py).
 *   - The unit of resampling is the test triple.  Every sample carries the id of its unit, and in a replicate every
 *     sample of a unit carries the unit's weight: for classification a triple and its corruptions, for ranking its tail
 *     query and its head query.  Methods that are given the same unit ids and seed see the same resample (paired).
 *   - Replicate 0 is the identity: every weight is 1.  Its outputs are the point estimates.
 *   - Replicate b >= 1 is a Poisson(1) bootstrap.  The weight of unit u:
 *       c      = philox4x32_10(counter = (u, (b - 1) >> 2, RGCN_RESAMPLE_STREAM, 0), key = (seed low word, seed high word))
 *       word   = c[(b - 1) & 3]                       - one Philox call serves four replicates
 *       weight = #{k : word >= T[k]},  T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!),  k = 0 .. 12: a weight is 0 .. 13
 *     A weight is a pure function of (seed, b, u): no index table, no atomics, nothing drawn in sequence.  The total
 *     weight varies by replicate (mean num_units, variance num_units), which ratio statistics do not mind.
 */
#ifndef RGCN_RESAMPLE_H
#define RGCN_RESAMPLE_H

#include "rgcn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGCN_RESAMPLE_STREAM 0x52534D50u   /* counter word 2 of every resampling draw */
#define RGCN_RESAMPLE_LEVELS 13            /* entries of T: the largest weight */
#define RGCN_RESAMPLE_THRESHOLDS                                                                                  \
  { 1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u, 4294609777u, 4294923276u,       \
    4294962463u, 4294966817u, 4294967252u, 4294967292u, 4294967295u }
#define RGCN_RESAMPLE_TILE 1024            /* samples a workgroup of rgcn_resample_curves scans per step */
#define RGCN_RESAMPLE_MAX_SAMPLES 268435456 /* 2^28: 13 * 2^28 < 2^32, so a prefix weight is a uint32 and auc2 an int64 */
#define RGCN_RESAMPLE_MAX_REPLICATES 65535
#define RGCN_RESAMPLE_MAX_K 8              /* Hits@k thresholds per call of rgcn_resample_ranks */

/* Common to the three entry points.  RGCN_ERR_ARG: a negative size, num_units <= 0 or a NULL array that would be read
 * or written.  RGCN_ERR_RANGE: more than RGCN_RESAMPLE_MAX_SAMPLES samples, num_units > 2^31 - 1 (unit ids are int32),
 * replicates > RGCN_RESAMPLE_MAX_REPLICATES, nk > RGCN_RESAMPLE_MAX_K.  RGCN_ERR_ALIGN (checked last, before any HIP
 * call): int64 and double arrays 8, `unit` 16 and `label` / `tie_end` 4 in rgcn_resample_curves (read four samples at a
 * time), `unit` and `k_values` 4 elsewhere; the uint8 weight rows have no requirement.  A unit id outside
 * [0, num_units) is clamped to 0 and raises the sticky flag (rgcn_index_error_fetch). */

/* out uint8[replicates + 1, num_units]: out[b, u] = the weight of unit u in replicate b (row 0 all ones). */
int rgcn_resample_weights(int64_t num_units, int64_t replicates, int64_t seed, uint8_t* out, void* stream);

/* ROC / PR statistics of n samples ALREADY IN DESCENDING SCORE ORDER, per replicate r = 0 .. replicates.
 *
 * label uint8[n] (1 positive, 0 negative), unit int32[n], tie_end uint8[n]: 1 on the last sample of each run of equal
 * scores (so tie_end[n - 1] = 1; the samples after the last 1 would form no group).  cut in [0, n]: the number of
 * samples with score >= threshold.  With w_i the weight of sample i's unit, a GROUP a run of equal scores, p_g / q_g
 * the positive / negative weight of group g and TP_before / FP_before the positive / negative weight of all groups in
 * front of it:
 *   wp[r], wn[r]  total positive / negative weight
 *   auc2[r]       sum over groups of q_g (2 TP_before + p_g): AUC-ROC = auc2 / (2 wp wn), ties counted half
 *   ap[r]         (sum over groups of p_g (TP_before + p_g) / (TP_before + p_g + FP_before + q_g)) / wp: the step-wise
 *                 average precision (scikit-learn's).  Each term is one exact integer product (below 2^53 whenever
 *                 n * 13 < 2^26) and one division; the terms are summed per lane in walk order and then over a fixed
 *                 tree, and the sum is divided once: |ap - exact| <= (n + 2) 2^-53, and two calls give the same bits.
 *   tp[r], fp[r]  positive / negative weight of the first `cut` samples
 * All integer outputs are exact.  A replicate with wp == 0 or wn == 0 stores auc2 = 0 and ap = 0.0 (undefined: the
 * caller marks it).  n == 0 stores zeros everywhere.  No floating-point atomics. */
int rgcn_resample_curves(const uint8_t* label, const int32_t* unit, const uint8_t* tie_end, int64_t n, int64_t cut,
                         int64_t num_units, int64_t replicates, int64_t seed, int64_t* wp, int64_t* wn, int64_t* auc2,
                         double* ap, int64_t* tp, int64_t* fp, void* stream);

/* Ranking statistics of m queries, per replicate r = 0 .. replicates.  rank int64[m] (1-based; 1 <= rank < 2^31),
 * unit int32[m], k_values int32[nk], nk in [0, RGCN_RESAMPLE_MAX_K]:
 *   w_sum[r]          sum of w_i              MRR = rr_sum / w_sum, mean rank = rank_sum / w_sum,
 *   rank_sum[r]       sum of w_i rank_i       Hits@k = hits / w_sum
 *   hits[r * nk + j]  sum of w_i [rank_i <= k_values[j]]
 *   rr_sum[r]         sum of w_i / rank_i, a double: per lane in walk order, then over a fixed tree - the same bits every
 *                     call, |rr_sum - exact| <= (m + 2) 2^-53 rr_sum
 * m == 0 stores zeros.  The median rank is not a sum and is not resampled. */
int rgcn_resample_ranks(const int64_t* rank, const int32_t* unit, int64_t m, const int32_t* k_values, int nk,
                        int64_t num_units, int64_t replicates, int64_t seed, int64_t* w_sum, int64_t* rank_sum,
                        int64_t* hits, double* rr_sum, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RGCN_RESAMPLE_H */
