// Bootstrap resampling of the evaluation metrics (include/rgcn_resample.h).
//
// The reference's `statistical_significance_test` (src/compare_methods.py:701-740) has no resampling at all; on the
// host one replicate of scikit-learn's weighted roc_auc_score + average_precision_score re-sorts the scores.  Here
// the scores are sorted ONCE (by the caller), and a replicate is a walk of that order under other integer weights:
// one workgroup per group of four replicates - the four words of one Philox call per unit - scans the list in tiles
// of RGCN_RESAMPLE_TILE samples.  A prefix weight is below 13 * 2^28 < 2^32, so the positive and the negative prefix
// travel as ONE uint64 (positives in the high word, negatives in the low one; the low word never carries), and one
// 64-bit scan does both.  The prefix in front of a tie group is the prefix at the previous tie_end; both words only
// grow along the list, so the packed values are ordered like the positions and that lookup is an exclusive max-scan.
// The sorted arrays (6 bytes per sample) are read by every workgroup and stay in L2.
#include "rgcn_common.h"
#include "rgcn_sample_core.h"
#include "../../include/rgcn_resample.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kPer = 4, kTile = kThreads * kPer, kReps = 4;
static_assert(kTile == RGCN_RESAMPLE_TILE, "the tile the header publishes");
static_assert((uint64_t)RGCN_RESAMPLE_LEVELS * RGCN_RESAMPLE_MAX_SAMPLES < ((uint64_t)1 << 32), "a prefix weight is a uint32");

__device__ inline uint32_t poisson_weight(uint32_t word) {
  constexpr uint32_t T[RGCN_RESAMPLE_LEVELS] = RGCN_RESAMPLE_THRESHOLDS;
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < RGCN_RESAMPLE_LEVELS; ++k) w += word >= T[k] ? 1u : 0u;
  return w;
}

// The replicates of workgroup (or grid row) `blk`: 0 is replicate 0 alone, the identity; blk >= 1 is the group
// blk - 1 of the rule, replicates 4 (blk - 1) + 1 .. + 4, as many of them as exist.
struct rep_group {
  uint32_t grp;
  int64_t first;
  int live;
};
__device__ inline rep_group group_of(unsigned blk, int64_t replicates) {
  if (blk == 0) return {0u, 0, 1};
  const int64_t first = 4 * (int64_t)(blk - 1) + 1, left = replicates - first + 1;
  return {blk - 1, first, (int)(left < kReps ? left : kReps)};
}

// the weights of unit u in the four replicates of a group
__device__ inline void group_weights(bool identity, uint32_t u, uint32_t grp, uint32_t k0, uint32_t k1, uint32_t (&w)[kReps]) {
  uint32_t c[4] = {u, grp, RGCN_RESAMPLE_STREAM, 0u};
  philox4x32_10(c, k0, k1);
#pragma unroll
  for (int r = 0; r < kReps; ++r) w[r] = identity ? (r == 0 ? 1u : 0u) : poisson_weight(c[r]);   // one workgroup's waste
}

__device__ inline uint32_t checked_unit(int32_t u, int64_t num_units, int* __restrict__ flag) {
  if ((uint64_t)(int64_t)u >= (uint64_t)num_units) {
    *flag = 1;
    u = 0;
  }
  return (uint32_t)u;
}

__device__ inline uint64_t wave_scan_sum(uint64_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up((unsigned long long)v, o);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ inline uint64_t wave_scan_max(uint64_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up((unsigned long long)v, o);
    if (lane >= o && t > v) v = t;
  }
  return v;
}
// butterfly sums: every lane ends with the same bits (a + b and b + a are the same double)
__device__ inline int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((long long)v, o);
  return v;
}
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kThreads) void k_resample_weights(int64_t num_units, int64_t replicates, uint32_t k0, uint32_t k1,
                                                               uint8_t* __restrict__ out) {
  const int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (u >= num_units) return;
  const rep_group g = group_of(blockIdx.y, replicates);
  uint32_t w[kReps];
  group_weights(blockIdx.y == 0, (uint32_t)u, g.grp, k0, k1, w);
#pragma unroll
  for (int r = 0; r < kReps; ++r)
    if (r < g.live) out[(g.first + r) * num_units + u] = (uint8_t)w[r];
}

__global__ __launch_bounds__(kThreads) void k_resample_curves(
    const uint8_t* __restrict__ label, const int32_t* __restrict__ unit, const uint8_t* __restrict__ tie_end, int64_t n,
    int64_t cut, int64_t num_units, int64_t replicates, uint32_t k0, uint32_t k1, int64_t* __restrict__ wp,
    int64_t* __restrict__ wn, int64_t* __restrict__ auc2, double* __restrict__ ap, int64_t* __restrict__ tp,
    int64_t* __restrict__ fp, int* __restrict__ flag) {
  __shared__ uint64_t s_sum[kWaves][kReps], s_max[kWaves][kReps], s_total[kReps];
  __shared__ int64_t s_auc[kWaves][kReps];
  __shared__ double s_ap[kWaves][kReps];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const rep_group g = group_of(blockIdx.x, replicates);
  const bool identity = blockIdx.x == 0;

  uint64_t carry[kReps] = {}, tie_carry[kReps] = {};   // the prefix in front of the tile; the prefix at the last tie_end
  int64_t auc[kReps] = {};
  double aps[kReps] = {};

  for (int64_t base = 0; base < n; base += kTile) {
    const int64_t i0 = base + (int64_t)tid * kPer;
    uint32_t lab[kPer], te[kPer];
    int32_t un[kPer];
    if (i0 + kPer <= n) {
      const uint32_t lw = *reinterpret_cast<const uint32_t*>(label + i0), tw = *reinterpret_cast<const uint32_t*>(tie_end + i0);
      const int4 uw = *reinterpret_cast<const int4*>(unit + i0);
      un[0] = uw.x; un[1] = uw.y; un[2] = uw.z; un[3] = uw.w;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        lab[j] = (lw >> (8 * j)) & 0xffu;
        te[j] = (tw >> (8 * j)) & 0xffu;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const bool in = i0 + j < n;
        lab[j] = in ? label[i0 + j] : 0u;
        te[j] = in ? tie_end[i0 + j] : 0u;
        un[j] = in ? unit[i0 + j] : 0;
      }
    }
    // the lane's own inclusive prefixes, (positive weight << 32) + negative weight
    uint64_t pre[kPer][kReps];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      uint32_t w[kReps] = {};
      if (i0 + j < n) group_weights(identity, checked_unit(un[j], num_units, flag), g.grp, k0, k1, w);
#pragma unroll
      for (int r = 0; r < kReps; ++r) {
        const uint64_t v = lab[j] ? (uint64_t)w[r] << 32 : (uint64_t)w[r];
        pre[j][r] = j ? pre[j - 1][r] + v : v;
      }
    }
    uint64_t incl[kReps];
#pragma unroll
    for (int r = 0; r < kReps; ++r) {
      incl[r] = wave_scan_sum(pre[kPer - 1][r], lane);
      if (lane == 63) s_sum[wave][r] = incl[r];
    }
    __syncthreads();
    uint64_t lane_max[kReps];
#pragma unroll
    for (int r = 0; r < kReps; ++r) {
      uint64_t front = carry[r] + (incl[r] - pre[kPer - 1][r]), all = carry[r];
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const uint64_t s = s_sum[w][r];
        if (w < wave) front += s;
        all += s;
      }
      carry[r] = all;
      lane_max[r] = 0;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        pre[j][r] += front;                              // now the prefix from the head of the list
        if (te[j]) lane_max[r] = pre[j][r];
      }
    }
    // the prefix at the last tie_end in front of the lane's first sample
    uint64_t prev[kReps];
#pragma unroll
    for (int r = 0; r < kReps; ++r) {
      const uint64_t m = wave_scan_max(lane_max[r], lane);
      if (lane == 63) s_max[wave][r] = m;
      const uint64_t up = __shfl_up((unsigned long long)m, 1);
      prev[r] = lane ? up : 0;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kReps; ++r) {
      uint64_t all = tie_carry[r];
      if (all > prev[r]) prev[r] = all;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const uint64_t s = s_max[w][r];
        if (w < wave && s > prev[r]) prev[r] = s;
        if (s > all) all = s;
      }
      tie_carry[r] = all;
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (i0 + j == cut - 1) {
#pragma unroll
        for (int r = 0; r < kReps; ++r)
          if (r < g.live) {
            tp[g.first + r] = (int64_t)(pre[j][r] >> 32);
            fp[g.first + r] = (int64_t)(pre[j][r] & 0xffffffffull);
          }
      }
      if (!te[j]) continue;
#pragma unroll
      for (int r = 0; r < kReps; ++r) {
        const uint64_t P = pre[j][r] >> 32, N = pre[j][r] & 0xffffffffull;
        const uint64_t P0 = prev[r] >> 32, N0 = prev[r] & 0xffffffffull;
        const uint64_t pg = P - P0, qg = N - N0;
        auc[r] += (int64_t)(qg * (2 * P0 + pg));
        if (pg) aps[r] += (double)(pg * P) / (double)(P + N);
        prev[r] = pre[j][r];
      }
    }
  }

#pragma unroll
  for (int r = 0; r < kReps; ++r) {
    const int64_t a = wave_sum(auc[r]);
    const double d = wave_sum(aps[r]);
    if (lane == 0) {
      s_auc[wave][r] = a;
      s_ap[wave][r] = d;
    }
    if (tid == 0) s_total[r] = carry[r];
  }
  __syncthreads();
  if (tid < g.live) {
    const int r = tid;
    const int64_t P = (int64_t)(s_total[r] >> 32), N = (int64_t)(s_total[r] & 0xffffffffull);
    int64_t a = 0;
    double d = 0.0;
    for (int w = 0; w < kWaves; ++w) {
      a += s_auc[w][r];
      d += s_ap[w][r];
    }
    const bool defined = P > 0 && N > 0;
    wp[g.first + r] = P;
    wn[g.first + r] = N;
    auc2[g.first + r] = defined ? a : 0;
    ap[g.first + r] = defined ? d / (double)P : 0.0;
    if (cut <= 0) {
      tp[g.first + r] = 0;
      fp[g.first + r] = 0;
    }
  }
}

constexpr int kRankSlots = 3 + RGCN_RESAMPLE_MAX_K;     // w_sum, rank_sum, hits[8], rr_sum

__global__ __launch_bounds__(kThreads) void k_resample_ranks(
    const int64_t* __restrict__ rank, const int32_t* __restrict__ unit, int64_t m, const int32_t* __restrict__ k_values, int nk,
    int64_t num_units, int64_t replicates, uint32_t k0, uint32_t k1, int64_t* __restrict__ w_sum,
    int64_t* __restrict__ rank_sum, int64_t* __restrict__ hits, double* __restrict__ rr_sum, int* __restrict__ flag) {
  __shared__ int64_t s_red[kWaves][kReps][kRankSlots];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const rep_group g = group_of(blockIdx.x, replicates);
  const bool identity = blockIdx.x == 0;
  int64_t kv[RGCN_RESAMPLE_MAX_K];
#pragma unroll
  for (int j = 0; j < RGCN_RESAMPLE_MAX_K; ++j) kv[j] = j < nk ? (int64_t)k_values[j] : INT64_MIN;
  int64_t ws[kReps] = {}, rs[kReps] = {}, hs[kReps][RGCN_RESAMPLE_MAX_K] = {};
  double rr[kReps] = {};
  for (int64_t i = tid; i < m; i += kThreads) {
    const int64_t rk = rank[i];
    uint32_t w[kReps];
    group_weights(identity, checked_unit(unit[i], num_units, flag), g.grp, k0, k1, w);
    const double inv_base = (double)rk;
#pragma unroll
    for (int r = 0; r < kReps; ++r) {
      ws[r] += w[r];
      rs[r] += (int64_t)w[r] * rk;
      if (w[r]) rr[r] += (double)w[r] / inv_base;
#pragma unroll
      for (int j = 0; j < RGCN_RESAMPLE_MAX_K; ++j) hs[r][j] += rk <= kv[j] ? (int64_t)w[r] : 0;
    }
  }
#pragma unroll
  for (int r = 0; r < kReps; ++r) {
    int64_t v[kRankSlots];
    v[0] = wave_sum(ws[r]);
    v[1] = wave_sum(rs[r]);
#pragma unroll
    for (int j = 0; j < RGCN_RESAMPLE_MAX_K; ++j) v[2 + j] = wave_sum(hs[r][j]);
    v[kRankSlots - 1] = __double_as_longlong(wave_sum(rr[r]));
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < kRankSlots; ++q) s_red[wave][r][q] = v[q];
    }
  }
  __syncthreads();
  if (tid >= kReps * kRankSlots) return;
  const int r = tid / kRankSlots, q = tid % kRankSlots;
  if (r >= g.live) return;
  const int64_t row = g.first + r;
  if (q == kRankSlots - 1) {
    double d = 0.0;
    for (int w = 0; w < kWaves; ++w) d += __longlong_as_double(s_red[w][r][q]);
    rr_sum[row] = d;
    return;
  }
  int64_t a = 0;
  for (int w = 0; w < kWaves; ++w) a += s_red[w][r][q];
  if (q == 0) w_sum[row] = a;
  else if (q == 1) rank_sum[row] = a;
  else if (q - 2 < nk) hits[row * nk + (q - 2)] = a;
}

inline int check_sizes(int64_t samples, int64_t num_units, int64_t replicates) {
  if (samples < 0 || num_units <= 0 || replicates < 0) return RGCN_ERR_ARG;
  if (samples > RGCN_RESAMPLE_MAX_SAMPLES || num_units > INT32_MAX || replicates > RGCN_RESAMPLE_MAX_REPLICATES)
    return RGCN_ERR_RANGE;
  return RGCN_OK;
}

// workgroups (or grid rows): replicate 0, then one per group of four
inline unsigned groups_of(int64_t replicates) { return 1u + (unsigned)ceil_div64(replicates, kReps); }

}  // namespace

extern "C" int rgcn_resample_weights(int64_t num_units, int64_t replicates, int64_t seed, uint8_t* out, void* stream_) {
  if (const int rc = check_sizes(0, num_units, replicates)) return rc;
  if (!out) return RGCN_ERR_ARG;
  const uint64_t s = (uint64_t)seed;
  dim3 grid((unsigned)ceil_div64(num_units, kThreads), groups_of(replicates));
  k_resample_weights<<<grid, kThreads, 0, (hipStream_t)stream_>>>(num_units, replicates, (uint32_t)s, (uint32_t)(s >> 32), out);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

extern "C" int rgcn_resample_curves(const uint8_t* label, const int32_t* unit, const uint8_t* tie_end, int64_t n, int64_t cut,
                                    int64_t num_units, int64_t replicates, int64_t seed, int64_t* wp, int64_t* wn,
                                    int64_t* auc2, double* ap, int64_t* tp, int64_t* fp, void* stream_) {
  if (const int rc = check_sizes(n, num_units, replicates)) return rc;
  if (cut < 0 || cut > n || !wp || !wn || !auc2 || !ap || !tp || !fp) return RGCN_ERR_ARG;
  if (n > 0 && (!label || !unit || !tie_end)) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(16, unit);
  RGCN_ALIGN_TRY(8, wp, wn, auc2, ap, tp, fp);
  RGCN_ALIGN_TRY(4, label, tie_end);
  int* flag = rgcn_index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  const uint64_t s = (uint64_t)seed;
  k_resample_curves<<<groups_of(replicates), kThreads, 0, (hipStream_t)stream_>>>(
      label, unit, tie_end, n, cut, num_units, replicates, (uint32_t)s, (uint32_t)(s >> 32), wp, wn, auc2, ap, tp, fp, flag);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

extern "C" int rgcn_resample_ranks(const int64_t* rank, const int32_t* unit, int64_t m, const int32_t* k_values, int nk,
                                   int64_t num_units, int64_t replicates, int64_t seed, int64_t* w_sum, int64_t* rank_sum,
                                   int64_t* hits, double* rr_sum, void* stream_) {
  if (const int rc = check_sizes(m, num_units, replicates)) return rc;
  if (nk < 0) return RGCN_ERR_ARG;
  if (nk > RGCN_RESAMPLE_MAX_K) return RGCN_ERR_RANGE;
  if (!w_sum || !rank_sum || !rr_sum || (nk > 0 && (!k_values || !hits))) return RGCN_ERR_ARG;
  if (m > 0 && (!rank || !unit)) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(8, rank, w_sum, rank_sum, hits, rr_sum);
  RGCN_ALIGN_TRY(4, unit, k_values);
  int* flag = rgcn_index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  const uint64_t s = (uint64_t)seed;
  k_resample_ranks<<<groups_of(replicates), kThreads, 0, (hipStream_t)stream_>>>(
      rank, unit, m, k_values, nk, num_units, replicates, (uint32_t)s, (uint32_t)(s >> 32), w_sum, rank_sum, hits, rr_sum, flag);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}
