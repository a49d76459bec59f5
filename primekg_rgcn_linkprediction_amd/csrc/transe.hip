// One batch-synchronous training step of the TransE baseline (include/rgcn_transe.h).
//
// Replaces the batch body of the reference's SimpleTransE.fit (src/compare_methods.py:229-270): `_compute_score` twice,
// the margin loss, the Python loop `for i in range(len(batch_indices)): if loss[i] > 0: ...` with its five row updates
// per sample, and `self.embeddings / np.linalg.norm(...)` over the whole table.  The reference's loop is serial (a later
// sample sees the rows an earlier one moved); here every difference is taken from the tables as the step finds them and
// a row's contributions are added in slot order and applied once - the ordered scatter of the DistMult backward
// (distmult.hip), taken from the header both files share (rgcn_ordered_match.h).  This file defines:
//   1. k_transe_contrib: one lane group of d/4 lanes per sample, float4 per lane, butterfly reduction of the two norms.
//      Writes the scaled rows 2 lr dp_i, 2 lr dn_i, the sample's loss, four int32 entity keys (-1 when the sample is
//      not active), the relation key and the relation row 2 lr (dp_i - dn_i) (exact zeros when not active).
//   2. k_transe_apply: one wave per slot.  A slot whose key occurs BEFORE it retires; the first occurrence adds the
//      signed rows of all occurrences in slot order, adds the sum to the table row, normalises it and writes it once.
//      A launch of its own: launch 1 reads the rows this one writes.
//   3. k_transe_loss: the mean loss in a fixed order and the two device-side accumulators.
// Between 2 and 3 the step launches the header's relation tree (k_segment_partials, k_segment_combine<true>: the
// combine pass subtracts the sum from the row).
// No floating-point atomics; two runs from the same tables give the same bits.
#include "rgcn_common.h"
#include "rgcn_ordered_match.h"
#include "../../include/rgcn_transe.h"

namespace {

constexpr int kThreads = 256;
constexpr int kApplyWaves = 16;                  // slots per workgroup of the apply launch: one staging of the keys serves sixteen
constexpr int kApplyKeysInLds = 8192;            // key count (4 per sample) up to which the apply launch stages the keys in LDS

__device__ inline float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ inline float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline float4 mul4(float s, float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
__device__ inline float dot4(float4 a) { return a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w; }

// dpn[2i] = 2 lr dp_i, dpn[2i + 1] = 2 lr dn_i, relrow[i] = 2 lr (dp_i - dn_i) or 0, loss[i], keys[4i .. 4i + 3], rkeys[i]
template <int G>
__global__ __launch_bounds__(kThreads) void k_transe_contrib(
    const float* __restrict__ emb, int64_t num_nodes, const float* __restrict__ rel, int64_t num_relations, int d,
    const int64_t* __restrict__ heads, const int64_t* __restrict__ tails, const int64_t* __restrict__ rels, int64_t B,
    float two_lr, float margin, float* __restrict__ dpn, float* __restrict__ relrow, float* __restrict__ loss,
    int32_t* __restrict__ keys, int32_t* __restrict__ rkeys, int* __restrict__ flag) {
  const int64_t b = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / G;
  const int gl = threadIdx.x % G;
  const bool live = b < B;                       // lanes past the batch stay for the butterflies
  int64_t h = 0, t = 0, hn = 0, tn = 0, r = 0;
  float sp = 0.f, sn = 0.f;
  // the host refuses a step without its id vectors: rgcn_checked_row's "no index vector, row b itself" cannot occur
  // here, and said so it costs no register
  __builtin_assume(heads != nullptr && tails != nullptr && rels != nullptr);
  if (live) {
    h = rgcn_checked_row(heads, b, num_nodes, flag);
    t = rgcn_checked_row(tails, b, num_nodes, flag);
    hn = rgcn_checked_row(heads, B + b, num_nodes, flag);
    tn = rgcn_checked_row(tails, B + b, num_nodes, flag);
    r = rgcn_checked_row(rels, b, num_relations, flag);
    for (int c = gl * 4; c < d; c += G * 4) {
      const float4 rv = ld4(rel + (size_t)r * d + c);
      const float4 dp = sub4(add4(ld4(emb + (size_t)h * d + c), rv), ld4(emb + (size_t)t * d + c));
      const float4 dn = sub4(add4(ld4(emb + (size_t)hn * d + c), rv), ld4(emb + (size_t)tn * d + c));
      sp += dot4(dp);
      sn += dot4(dn);
      *reinterpret_cast<float4*>(dpn + (size_t)(2 * b) * d + c) = mul4(two_lr, dp);
      *reinterpret_cast<float4*>(dpn + (size_t)(2 * b + 1) * d + c) = mul4(two_lr, dn);
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    sp += __shfl_xor(sp, off, G);
    sn += __shfl_xor(sn, off, G);
  }
  if (!live) return;
  const float x = margin + sqrtf(sp) - sqrtf(sn);
  const bool active = x > 0.f;                   // NaN: not active, but the loss keeps it
  if (gl == 0) {
    loss[b] = x <= 0.f ? 0.f : x;
    keys[4 * b + 0] = active ? (int32_t)h : -1;
    keys[4 * b + 1] = active ? (int32_t)t : -1;
    keys[4 * b + 2] = active ? (int32_t)hn : -1;
    keys[4 * b + 3] = active ? (int32_t)tn : -1;
    rkeys[b] = (int32_t)r;
  }
  // the relation row from the tables again (their lines are in L1): 2 lr (dp - dn) as the contract spells it
  for (int c = gl * 4; c < d; c += G * 4) {
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
      const float4 rv = ld4(rel + (size_t)r * d + c);
      const float4 dp = sub4(add4(ld4(emb + (size_t)h * d + c), rv), ld4(emb + (size_t)t * d + c));
      const float4 dn = sub4(add4(ld4(emb + (size_t)hn * d + c), rv), ld4(emb + (size_t)tn * d + c));
      out = mul4(two_lr, sub4(dp, dn));
    }
    *reinterpret_cast<float4*>(relrow + (size_t)b * d + c) = out;
  }
}

// keys[S] (S = 4B, -1: not active), dpn[2B, d] -> emb[key] = normalised(emb[key] + signed sum), once per key
template <bool IN_LDS>
__global__ __launch_bounds__(64 * kApplyWaves) void k_transe_apply(const int32_t* __restrict__ keys, int S,
                                                                   const float* __restrict__ dpn, int d,
                                                                   float* __restrict__ emb) {
  __shared__ int32_t skeys[IN_LDS ? kApplyKeysInLds : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* k = stage_keys<IN_LDS, 64 * kApplyWaves>(keys, S, skeys);
  const int s = blockIdx.x * kApplyWaves + wave;
  if (s >= S) return;
  const int my = k[s];
  if (my < 0) return;                            // a slot of a sample that is not active
  for (int c = 0; c < s; c += 64)               // an earlier occurrence owns the row
    if (earlier_slot_has(k, my, s, c, lane)) return;
  float* row = emb + (size_t)my * d;
  float ss = 0.f;
  for (int c0 = lane * 4; c0 < ((d + 255) & ~255); c0 += 256) {
    MatchIter it;
    it.start(k, my, s, S, lane);
    const int cc = min(c0, d - 4);               // lanes past the row stay for the iterator's ballots
    const float4 acc = ordered_row_sum<TranseRows>(it, dpn, d, cc, lane);
    if (c0 < d) {
      const float4 v = add4(ld4(row + c0), acc);
      ss += dot4(v);
      *reinterpret_cast<float4*>(row + c0) = v;  // read back below by the lane that wrote it
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
  const float norm = sqrtf(ss);
  for (int c0 = lane * 4; c0 < d; c0 += 256) {
    const float4 v = ld4(row + c0);
    *reinterpret_cast<float4*>(row + c0) = make_float4(v.x / norm, v.y / norm, v.z / norm, v.w / norm);
  }
}

// mean of the per-sample losses (thread i adds elements i, i + 1024, ..., then a fixed tree), the active count (a sample
// is active iff its first key is not -1) and the two running sums
__global__ __launch_bounds__(1024) void k_transe_loss(const float* __restrict__ loss, const int32_t* __restrict__ keys, int B,
                                                      float* __restrict__ loss_mean, double* __restrict__ loss_sum,
                                                      long long* __restrict__ active_sum) {
  const SumTally total = block1024_sum_tally(B, [&](int b, float& s, int& active) {
    s += loss[b];
    active += keys[4 * b] >= 0 ? 1 : 0;
  });
  if (threadIdx.x == 0) {
    const float mean = total.sum / (float)B;
    loss_mean[0] = mean;
    if (loss_sum) loss_sum[0] += (double)mean;
    if (active_sum) active_sum[0] += total.tally;
  }
}

// the workspace's sections, each on a 256-byte boundary
struct Layout {
  size_t dpn, relrow, partial, loss, keys, rkeys, bytes;
  int64_t nseg;
};

Layout layout(int64_t batch, int64_t d, int64_t R) {
  Layout l;
  l.nseg = ceil_div64(batch, segment_len(batch));
  size_t at = 0;
  l.dpn = at;     at = align256(at + (size_t)2 * batch * d * sizeof(float));
  l.relrow = at;  at = align256(at + (size_t)batch * d * sizeof(float));
  l.partial = at; at = align256(at + (size_t)l.nseg * R * d * sizeof(float));
  l.loss = at;    at = align256(at + (size_t)batch * sizeof(float));
  l.keys = at;    at = align256(at + (size_t)4 * batch * sizeof(int32_t));
  l.rkeys = at;   at = align256(at + (size_t)batch * sizeof(int32_t));
  l.bytes = at;
  return l;
}

constexpr int64_t kMaxBatch = (int64_t)1 << 28;  // 4 * batch slots are counted in an int

}  // namespace

extern "C" {

size_t rgcn_transe_step_workspace_bytes(int64_t batch, int64_t d, int64_t num_relations) {
  if (batch <= 0 || batch > kMaxBatch || d <= 0 || (d & 3) || num_relations <= 0 || num_relations > INT32_MAX) return 0;
  return layout(batch, d, num_relations).bytes;
}

int rgcn_transe_step(float* emb, int64_t num_nodes, float* rel, int64_t num_relations, int64_t d, const int64_t* heads,
                     const int64_t* tails, const int64_t* rels, int64_t batch, float lr, float margin, float* loss_mean,
                     double* loss_sum, int64_t* active_sum, void* workspace, size_t workspace_bytes, void* stream_) {
  if (batch < 0 || d <= 0 || (d & 3) || num_nodes <= 0 || num_relations <= 0) return RGCN_ERR_ARG;
  if (batch == 0) return RGCN_OK;
  if (!emb || !rel || !heads || !tails || !rels || !loss_mean || !workspace) return RGCN_ERR_ARG;
  if (num_nodes > INT32_MAX || num_relations > INT32_MAX || batch > kMaxBatch || d > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  const Layout l = layout(batch, d, num_relations);
  if (workspace_bytes < l.bytes) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(16, emb, rel, workspace);       // rows as float4; ids, the loss and the running sums one element at a time
  RGCN_ALIGN_TRY(8, heads, tails, rels, loss_sum, active_sum);
  RGCN_ALIGN_TRY(4, loss_mean);
  hipStream_t stream = (hipStream_t)stream_;
  int* flag = rgcn_index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  char* ws = (char*)workspace;
  float* dpn = (float*)(ws + l.dpn);
  float* relrow = (float*)(ws + l.relrow);
  float* partial = (float*)(ws + l.partial);
  float* loss = (float*)(ws + l.loss);
  int32_t* keys = (int32_t*)(ws + l.keys);
  int32_t* rkeys = (int32_t*)(ws + l.rkeys);
  const int g = rgcn_pick_group(d);
  const unsigned grid = (unsigned)ceil_div64(batch, kThreads / g);
  RGCN_DISPATCH_G(g, (k_transe_contrib<G><<<grid, kThreads, 0, stream>>>(emb, num_nodes, rel, num_relations, (int)d, heads,
                                                                        tails, rels, batch, 2.f * lr, margin, dpn, relrow,
                                                                        loss, keys, rkeys, flag)));
  const int S = (int)(4 * batch);
  const unsigned ag = (unsigned)ceil_div64(S, kApplyWaves);
  if (S <= kApplyKeysInLds) k_transe_apply<true><<<ag, 64 * kApplyWaves, 0, stream>>>(keys, S, dpn, (int)d, emb);
  else k_transe_apply<false><<<ag, 64 * kApplyWaves, 0, stream>>>(keys, S, dpn, (int)d, emb);
  dim3 pg((unsigned)num_relations, (unsigned)l.nseg);
  k_segment_partials<<<pg, 64, 0, stream>>>(rkeys, (int)batch, relrow, (int)d, (int)num_relations, (int)segment_len(batch),
                                            partial);
  k_segment_combine<true><<<(unsigned)num_relations, 64, 0, stream>>>(partial, (int)l.nseg, (int)num_relations, (int)d, rel);
  k_transe_loss<<<1, 1024, 0, stream>>>(loss, keys, (int)batch, loss_mean, loss_sum,
                                        reinterpret_cast<long long*>(active_sum));
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // extern "C"
