// Fixed-order sum of the parameter-gradient slabs (see k_gemm_tn_dma): shared by the standalone
// reduction launch (rgcn_transform.hip) and by the gather launch that can carry it as extra
// workgroups (rgcn_aggregate.hip) - in a layer's backward the slab GEMM is followed by a transposed
// gather that does not depend on it, so the 5 us reduction rides along instead of sitting between
// two launch boundaries.
//
// The reduction is all latency: a thread owns one float4 of the output and the S / 16 slabs of one group, 64 KB or more
// apart.  Its loads are independent of each other and only the adds have an order, so a group's slabs are requested in
// predicated batches of RGCN_SLAB_BATCH (absent slabs: no load, +0.0f) and then added in slab order: one memory round
// trip per batch whatever S is - C2's groups hold 3 or 4 slabs (conv2) and 7 or 8 (conv1), each group one batch.  The
// bias partials take the same loop with another base and stride.
#pragma once
#include "rgcn_common.h"

constexpr int RGCN_SLAB_OUTS = 16, RGCN_SLAB_GROUPS = 16;     // outputs (float4) x slab groups per workgroup
#ifndef RGCN_SLAB_BATCH
#define RGCN_SLAB_BATCH 8                                     // loads in flight per thread (4 and 16: profiles/slab_riders.txt)
#endif

// workgroups needed for one job (host)
static inline int64_t rgcn_slab_reduce_blocks(const rgcn_slab_job& J) {
  const int64_t nq = (int64_t)J.Kc * J.N / 4 + (J.grad_bias ? (J.N + 3) / 4 : 0);
  return ceil_div64(nq, RGCN_SLAB_OUTS);
}

// Workgroup `block` of the reduction.  OUTS outputs (float4 each) x GROUPS slab groups: group g sums
// slabs [g*S/GROUPS, (g+1)*S/GROUPS) in order, then the partials are added in group order through
// `red` (256 float4 of LDS).  Deterministic.
// The sum of a group starts at +0.0f and can never become -0.0f (x + y is -0 only for two -0 operands), so the +0.0f
// that stands in for an absent slab of the last batch leaves every bit of it as it was, a NaN or an infinity included.
// N is a multiple of 4 (every entry point that takes a job refuses another), so the bias outputs are whole float4 too:
// n + 3 < N holds for every n = 4 * (q - nq) < N, and no element-wise guard is left.
template <int OUTS, int GROUPS>
__device__ inline void rgcn_slab_reduce_block(const rgcn_slab_job& J, int64_t block, float4* red) {
  static_assert(OUTS * GROUPS == 256, "one thread per (output, slab group)");
  constexpr int B = RGCN_SLAB_BATCH;
  const int64_t nq = (int64_t)J.Kc * J.N / 4;                  // float4 outputs of the weight grads
  const int64_t q = block * OUTS + ((int)threadIdx.x % OUTS);
  const int grp = (int)threadIdx.x / OUTS;
  const int S = J.splits, N = J.N;
  const int s0 = (int)((int64_t)S * grp / GROUPS), s1 = (int)((int64_t)S * (grp + 1) / GROUPS);
  const bool is_bias = q >= nq && J.grad_bias && q - nq < N / 4;   // tail outputs: bias partials
  const float* p = nullptr;                                    // the thread's float4 of slab 0; `stride` floats per slab
  size_t stride = 0;
  if (q < nq) {
    p = J.slab + (size_t)q * 4;
    stride = (size_t)J.Kc * N;
  } else if (is_bias) {
    p = J.bias_part + (size_t)(q - nq) * 4;
    stride = (size_t)N;
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p) {
    for (int i = s0; i < s1; i += B) {
      float4 v[B];
#pragma unroll
      for (int u = 0; u < B; ++u) {
        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i + u < s1) v[u] = *reinterpret_cast<const float4*>(p + (size_t)(i + u) * stride);
      }
#pragma unroll
      for (int u = 0; u < B; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (grp != 0) return;
  float4 s = red[threadIdx.x];
#pragma unroll
  for (int g = 1; g < GROUPS; ++g) {
    const float4 v = red[g * OUTS + threadIdx.x];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  if (q < nq) {
    const int64_t e = q * 4, k1n = (int64_t)J.K1 * N;
    if (e < k1n) *reinterpret_cast<float4*>(J.grad_weight + e) = s;
    else if (J.grad_root) *reinterpret_cast<float4*>(J.grad_root + (e - k1n)) = s;
  } else if (is_bias) {
    *reinterpret_cast<float4*>(J.grad_bias + (q - nq) * 4) = s;
  }
}

// standalone launch body
__global__ __launch_bounds__(256) static void k_slab_reduce(const rgcn_slab_job J) {
  __shared__ float4 red[256];
  rgcn_slab_reduce_block<RGCN_SLAB_OUTS, RGCN_SLAB_GROUPS>(J, blockIdx.x, red);
}
