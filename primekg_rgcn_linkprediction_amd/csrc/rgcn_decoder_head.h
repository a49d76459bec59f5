// The frame of a decoder head: score(h, r, t) per triple, the optional BCE loss beside it, and the deterministic
// backward - everything in front of the ordered scatter (rgcn_ordered_match.h) that does not depend on the decoder.
// Users: distmult.hip (policy DistMult) and complex.hip (policy ComplEx).
//
// One lane group of G = rgcn_pick_group(columns) lanes per triple, float4 per lane and trip, wavefront butterfly
// (__shfl_xor) reduction over the group - no LDS, no intermediate [B, d] tensors.
//
// Backward, deterministic (no float atomics): duplicates in head / tail / relation ids are legal and frequent (a hub
// is the head or tail of dozens of a 2,048-sample batch; 3 relation rows take them all).
//   1. k_head_contrib: per sample the decoder's three gradient rows - into the caller's buffer for an operand without
//      an index (row b is its own), otherwise into workspace rows, and the sample's row ids as int32 keys.  Rider
//      workgroups behind the working ones clear the gradient tables the scatter writes rows into (zero_tables).
//   2. k_scatter_rows: one wave per slot (a head or tail occurrence); the first occurrence of a row adds the workspace
//      rows of all its occurrences in slot order and writes the row once.  Head and tail slots of one table
//      (grad_h == grad_t) are one key space.
//   3. k_segment_partials / k_segment_combine: the relation table (few rows, hundreds of occurrences each) as a fixed
//      two-level tree.
// Every sum has a fixed order: two runs give the same bits.
//
// A decoder policy `Dec` supplies only what differs:
//   static constexpr int kWidth                      the multiple the row width d must have (4 or 8)
//   static int columns(int d)                        the float columns a lane group walks, four per lane and trip
//   __device__ static void score(hp, rp, tp, c, d, s)
//                                                    add the trip at column c of the triple's rows to the score s
//   __device__ static void contrib(g, hp, rp, tp, c, d, out_h, out_t, out_r, bo)
//                                                    store the trip at column c of the three gradient rows of a sample
//                                                    with upstream gradient g, each at out_* + bo unless out_* is NULL
// tests/test_head_parent_bits.py holds both heads to the bytes they gave before this frame existed: hipcc contracts
// a * b + c by how the expression reaches it, so a policy keeps its products written as they are.
// Everything sits in an anonymous namespace: each translation unit gets its own copies, the kernels included.
#pragma once
#include "rgcn_common.h"
#include "rgcn_ordered_match.h"

namespace {

constexpr int kHeadThreads = 256;

// binary_cross_entropy_with_logits per element, the way aten evaluates it
// ((1 - y) * x - log_sigmoid(x), log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|))); reference use:
// nn.BCEWithLogitsLoss, src/train.py:139, 300.
__device__ inline float bce_with_logits(float x, float y) {
  return (1.f - y) * x - (fminf(x, 0.f) - log1pf(expf(-fabsf(x))));
}

// `flag`: the library's sticky index-error flag (rgcn_index_error_flag) - a parameter, since the symbol lives in one
// object and this header in two
template <class Dec, int G, bool BCE>
__global__ __launch_bounds__(kHeadThreads) void k_head_fwd(const float* __restrict__ h, const int64_t* __restrict__ hi,
                                                           int64_t h_rows, const float* __restrict__ t,
                                                           const int64_t* __restrict__ ti, int64_t t_rows,
                                                           const float* __restrict__ r, const int64_t* __restrict__ ri,
                                                           int64_t r_rows, int64_t B, int d, float* __restrict__ scores,
                                                           int* __restrict__ flag, const float* __restrict__ labels,
                                                           float* __restrict__ loss) {
  const int64_t b = ((int64_t)blockIdx.x * kHeadThreads + threadIdx.x) / G;
  const int gl = threadIdx.x % G;
  const bool live = b < B;                       // lanes past the batch stay for the butterfly
  const int n = Dec::columns(d);
  float s = 0.f;
  if (live) {
    const float* hp = h + (size_t)rgcn_checked_row(hi, b, h_rows, flag) * d;
    const float* tp = t + (size_t)rgcn_checked_row(ti, b, t_rows, flag) * d;
    const float* rp = r + (size_t)rgcn_checked_row(ri, b, r_rows, flag) * d;
    for (int c = gl * 4; c < n; c += G * 4) Dec::score(hp, rp, tp, c, d, s);
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, G);
  if (live && gl == 0) {
    scores[b] = s;
    if (BCE) loss[b] = bce_with_logits(s, labels[b]);
  }
}

template <class Dec, int G, bool BCE>
__global__ __launch_bounds__(kHeadThreads) void k_head_contrib(
    const float* __restrict__ gs, const float* __restrict__ h, const int64_t* __restrict__ hi, int64_t h_rows,
    const float* __restrict__ t, const int64_t* __restrict__ ti, int64_t t_rows, const float* __restrict__ r,
    const int64_t* __restrict__ ri, int64_t r_rows, int64_t B, int d, float* __restrict__ out_h,
    float* __restrict__ out_t, float* __restrict__ out_r, int32_t* __restrict__ key_h, int32_t* __restrict__ key_t,
    int32_t* __restrict__ key_r, const float* __restrict__ scores, const float* __restrict__ labels, int work_blocks,
    float* __restrict__ zero_a, int64_t zero_a_quads, float* __restrict__ zero_b, int64_t zero_b_quads,
    int* __restrict__ flag) {
  if ((int)blockIdx.x >= work_blocks) {          // riders: zero the gradient tables the scatter launch writes rows into
    const int64_t stride = (int64_t)(gridDim.x - work_blocks) * kHeadThreads;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t q = (int64_t)((int)blockIdx.x - work_blocks) * kHeadThreads + threadIdx.x; q < zero_a_quads + zero_b_quads; q += stride) {
      if (q < zero_a_quads) reinterpret_cast<float4*>(zero_a)[q] = z;
      else reinterpret_cast<float4*>(zero_b)[q - zero_a_quads] = z;
    }
    return;
  }
  const int64_t b = ((int64_t)blockIdx.x * kHeadThreads + threadIdx.x) / G;
  const int gl = threadIdx.x % G;
  if (b >= B) return;
  const int64_t hr = rgcn_checked_row(hi, b, h_rows, flag), tr = rgcn_checked_row(ti, b, t_rows, flag),
                rr = rgcn_checked_row(ri, b, r_rows, flag);
  if (gl == 0) {
    if (key_h) key_h[b] = (int32_t)hr;
    if (key_t) key_t[b] = (int32_t)tr;
    if (key_r) key_r[b] = (int32_t)rr;
  }
  const int n = Dec::columns(d);
  const size_t ho = (size_t)hr * d, to = (size_t)tr * d, ro = (size_t)rr * d, bo = (size_t)b * d;
  const float g = BCE ? gs[0] * (1.f / (1.f + expf(-scores[b])) - labels[b]) / (float)B : gs[b];
  for (int c = gl * 4; c < n; c += G * 4) Dec::contrib(g, h + ho, r + ro, t + to, c, d, out_h, out_t, out_r, bo);
}

template <class Dec, bool BCE>
int head_fwd_impl(const float* h, const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx, int64_t t_rows,
                  const float* r, const int64_t* r_idx, int64_t r_rows, const float* labels, int64_t batch, int64_t d,
                  float* scores, float* loss, hipStream_t stream) {
  if (batch < 0 || d <= 0 || (d % Dec::kWidth) || h_rows < 0 || t_rows < 0 || r_rows < 0) return RGCN_ERR_ARG;
  if (batch == 0) return RGCN_OK;
  if (!h || !t || !r || !scores || (BCE && (!labels || !loss))) return RGCN_ERR_ARG;
  if (d > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  RGCN_ALIGN_TRY(16, h, t, r);
  RGCN_ALIGN_TRY(8, h_idx, t_idx, r_idx);
  RGCN_ALIGN_TRY(4, labels, scores, loss);
  int* flag = rgcn_index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  const int g = rgcn_pick_group(Dec::columns((int)d));
  const unsigned grid = (unsigned)ceil_div64(batch, kHeadThreads / g);
  RGCN_DISPATCH_G(g, (k_head_fwd<Dec, G, BCE><<<grid, kHeadThreads, 0, stream>>>(h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx,
                                                                               r_rows, batch, (int)d, scores, flag, labels, loss)));
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

// bytes of the backward's workspace: three [batch, d] contribution buffers, the relation tree's partial sums, three
// key vectors.  r_rows: 0 for a relation operand without an index.
inline size_t head_bwd_workspace_bytes(int64_t batch, int64_t d, int64_t r_rows) {
  if (batch <= 0 || d <= 0) return 0;
  const int64_t nseg = ceil_div64(batch, segment_len(batch));
  return ((size_t)3 * batch * d + (size_t)nseg * (r_rows > 0 ? r_rows : 0) * d) * sizeof(float) +
         (size_t)3 * batch * sizeof(int32_t) + 256;
}

// BCE: gs is the one-element gradient of the mean loss and the coefficient per sample comes from scores and labels
template <class Dec, bool BCE>
int head_bwd_impl(const float* gs, const float* scores, const float* labels, const float* h, const int64_t* h_idx,
                  int64_t h_rows, const float* t, const int64_t* t_idx, int64_t t_rows, const float* r, const int64_t* r_idx,
                  int64_t r_rows, int64_t batch, int64_t d, float* grad_h, float* grad_t, float* grad_r, void* workspace,
                  size_t workspace_bytes, int zero_tables, hipStream_t stream) {
  if (batch < 0 || d <= 0 || (d % Dec::kWidth) || h_rows < 0 || t_rows < 0 || r_rows < 0) return RGCN_ERR_ARG;
  if (batch == 0) {
    // no launch to carry the riders: an empty batch still owes its caller cleared (indexed) gradient tables
    // (every buffer whole: the index vectors of an empty batch arrive as NULL, so "indexed" cannot be told here)
    if (zero_tables) {
      if (grad_h && h_rows) RGCN_HIP_TRY(hipMemsetAsync(grad_h, 0, (size_t)h_rows * d * sizeof(float), stream));
      if (grad_t && t_rows && grad_t != grad_h) RGCN_HIP_TRY(hipMemsetAsync(grad_t, 0, (size_t)t_rows * d * sizeof(float), stream));
      if (grad_r && r_rows) RGCN_HIP_TRY(hipMemsetAsync(grad_r, 0, (size_t)r_rows * d * sizeof(float), stream));
    }
    return RGCN_OK;
  }
  if (!gs || !h || !t || !r || (BCE && (!scores || !labels))) return RGCN_ERR_ARG;
  if (batch > INT32_MAX / 4 || h_rows > INT32_MAX || t_rows > INT32_MAX || r_rows > INT32_MAX || d > INT32_MAX)
    return RGCN_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < head_bwd_workspace_bytes(batch, d, r_idx ? r_rows : 0)) return RGCN_ERR_WORKSPACE;
  RGCN_ALIGN_TRY(16, h, t, r, grad_h, grad_t, grad_r, workspace);
  RGCN_ALIGN_TRY(8, h_idx, t_idx, r_idx);
  RGCN_ALIGN_TRY(4, gs, scores, labels);
  int* flag = rgcn_index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  float* ws = (float*)workspace;
  const size_t bd = (size_t)batch * d;
  float *ch = ws, *ct = ws + bd, *cr = ws + 2 * bd;
  const int64_t nseg = ceil_div64(batch, segment_len(batch));
  float* partial = ws + 3 * bd;
  int32_t* keys = (int32_t*)(partial + (size_t)nseg * (r_idx ? r_rows : 0) * d);
  int32_t *kh = keys, *kt = keys + batch, *kr = keys + 2 * batch;
  // an operand without an index: row b is its own, written straight to the caller's buffer
  float* out_h = grad_h ? (h_idx ? ch : grad_h) : nullptr;
  float* out_t = grad_t ? (t_idx ? ct : grad_t) : nullptr;
  float* out_r = grad_r ? (r_idx ? cr : grad_r) : nullptr;
  const int g = rgcn_pick_group(Dec::columns((int)d));
  const unsigned grid = (unsigned)ceil_div64(batch, kHeadThreads / g);
  const bool sh = grad_h && h_idx, st = grad_t && t_idx;
  // zero_tables: the tables the scatter below writes rows into are cleared by riders of this launch (the relation
  // table is written whole by its tree)
  float *za = nullptr, *zb = nullptr;
  int64_t zaq = 0, zbq = 0;
  if (zero_tables) {
    if (sh) { za = grad_h; zaq = h_rows * d / 4; }
    if (st && !(sh && grad_h == grad_t)) { zb = grad_t; zbq = t_rows * d / 4; }
  }
  const unsigned riders = (zaq + zbq) > 0 ? (unsigned)std::min<int64_t>(1024, ceil_div64(zaq + zbq, 4 * kHeadThreads)) : 0u;
  RGCN_DISPATCH_G(g, (k_head_contrib<Dec, G, BCE><<<grid + riders, kHeadThreads, 0, stream>>>(
                    gs, h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows, batch, (int)d, out_h, out_t, out_r,
                    sh ? kh : nullptr, st ? kt : nullptr, (grad_r && r_idx) ? kr : nullptr, scores, labels, (int)grid, za,
                    zaq, zb, zbq, flag)));
  if (sh && st && grad_h == grad_t) {            // one table, one key space: head slots then tail slots
    rgcn_scatter_rows(kh, (int)(2 * batch), ch, (int)d, grad_h, stream);
  } else {
    if (sh) rgcn_scatter_rows(kh, (int)batch, ch, (int)d, grad_h, stream);
    if (st) rgcn_scatter_rows(kt, (int)batch, ct, (int)d, grad_t, stream);
  }
  if (grad_r && r_idx && r_rows > 0) {
    dim3 pg((unsigned)r_rows, (unsigned)nseg);
    k_segment_partials<<<pg, 64, 0, stream>>>(kr, (int)batch, cr, (int)d, (int)r_rows, (int)segment_len(batch), partial);
    k_segment_combine<false><<<(unsigned)r_rows, 64, 0, stream>>>(partial, (int)nseg, (int)r_rows, (int)d, grad_r);
  }
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace
