// DistMult edge-scoring head: scores[b] = sum_d H[hi(b), d] * R[ri(b), d] * T[ti(b), d].
//
// Replaces the reference's two row gathers `node_embeddings[head_indices]`,
// `node_embeddings[tail_indices]` (src/models/rgcn.py:325-326), the
// relation-embedding lookup and `torch.sum(h * r * t, dim=1)` (rgcn.py:207-211, row C2), and
// their autograd.  The kernels, the argument checks, the workspace layout and the deterministic backward are the
// decoder-head frame's (rgcn_decoder_head.h, shared with complex.hip); this file is the DistMult policy - one lane
// group of G = d/4 lanes per triple, the three products of a float4 column - and the entry points that pick the
// frame's instances.  It also keeps what every head shares as ONE symbol: the sticky index-error flag, the loss
// reduction (k_bce_reduce) and rgcn_segment_sum.
#include "rgcn_common.h"
#include "rgcn_decoder_head.h"

namespace {

// Sticky per-device flag: some kernel of this library met an index outside its table.  Indices are
// clamped before they are used (nothing is ever dereferenced out of bounds) and the flag is raised;
// rgcn_index_error_fetch reads and clears it (the reference's torch indexing raises a device-side assert
// in the same situation, asynchronously; an error CODE would need a host sync per call).
__device__ int g_index_error = 0;

// The policy of the frame - what a decoder must supply (rgcn_decoder_head.h has the list): the width multiple kWidth,
// the columns a lane group walks, one trip of the score and one trip of the three gradient rows.  Here: d real columns,
// the width a multiple of 4.
struct DistMult {
  static constexpr int kWidth = 4;
  __host__ __device__ static inline int columns(int d) { return d; }
  __device__ static inline void score(const float* hp, const float* rp, const float* tp, int c, int, float& s) {
    const float4 a = ld4(hp + c), m = ld4(rp + c), z = ld4(tp + c);
    s += a.x * m.x * z.x;
    s += a.y * m.y * z.y;
    s += a.z * m.z * z.z;
    s += a.w * m.w * z.w;
  }
  // the gradient rows g*r*t, g*h*r, g*h*t
  __device__ static inline void contrib(float g, const float* hp, const float* rp, const float* tp, int c, int,
                                        float* out_h, float* out_t, float* out_r, size_t bo) {
    const float4 a = ld4(hp + c), m = ld4(rp + c), z = ld4(tp + c);
    if (out_h) *reinterpret_cast<float4*>(out_h + bo + c) = make_float4(g * m.x * z.x, g * m.y * z.y, g * m.z * z.z, g * m.w * z.w);
    if (out_t) *reinterpret_cast<float4*>(out_t + bo + c) = make_float4(g * a.x * m.x, g * a.y * m.y, g * a.z * m.z, g * a.w * m.w);
    if (out_r) *reinterpret_cast<float4*>(out_r + bo + c) = make_float4(g * a.x * z.x, g * a.y * z.y, g * a.z * z.z, g * a.w * z.w);
  }
};


// The step's bookkeeping in ONE launch (one 1,024-thread workgroup): mean of the per-sample losses (fixed order: thread i
// adds elements i, i + 1024, ... , then a fixed tree - two runs give the same bits), the epoch's running sums
// (src/train.py:321-326: `predictions = sigmoid(scores) > 0.5`, `correct += (predictions == labels).sum()`,
// `total_loss += loss.item() * labels.size(0)`) kept on the device, and the batch cursor moved on.
// The prediction here is the SIGN of the score, `s > 0` (NaN and both zeros predict 0).  That is the reference's
// expression for every score outside 0 < s < 2^-23.  Inside that window fp32 sigmoid(s) may round to exactly 0.5
// (torch's does up to about 6e-8) and the reference then predicts 0: the kernel predicts 1 (it does not reproduce
// the rounding of torch's expf).
__global__ __launch_bounds__(1024) void k_bce_reduce(const float* __restrict__ loss, const float* __restrict__ scores,
                                                     const float* __restrict__ labels, int B, float* __restrict__ mean_loss,
                                                     double* __restrict__ loss_sum, long long* __restrict__ correct,
                                                     long long* __restrict__ cursor, long long cursor_add) {
  const SumTally total = block1024_sum_tally(B, [&](int b, float& s, int& hits) {
    s += loss[b];
    if (correct) hits += ((scores[b] > 0.f) == (labels[b] > 0.5f)) ? 1 : 0;
  });
  if (threadIdx.x == 0) {
    const float mean = total.sum / (float)B;
    mean_loss[0] = mean;
    if (loss_sum) loss_sum[0] += (double)mean * (double)B;
    if (correct) correct[0] += total.tally;
    if (cursor) cursor[0] += cursor_add;
  }
}

__global__ void k_keys32(const int64_t* __restrict__ idx, int64_t B, int64_t rows, int32_t* __restrict__ keys) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) keys[b] = (int32_t)rgcn_checked_row(idx, b, rows, &g_index_error);
}

}  // namespace

// The flag's address on the current device, looked up once per device and kept: the lookup (hipGetSymbolAddress) is not
// a stream operation, so a call that is being captured into a HIP graph must not be the device's first (rgcn_common.h).
int* rgcn_index_error_flag() {
  static int* flags[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  const bool kept = dev >= 0 && dev < 64;
  if (kept && flags[dev]) return flags[dev];
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_index_error)) != hipSuccess) return nullptr;
  if (kept) flags[dev] = static_cast<int*>(p);
  return static_cast<int*>(p);
}

extern "C" {

int rgcn_index_error_fetch(int* host_flag, void* stream_) {
  if (!host_flag) return RGCN_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  int zero = 0;
  RGCN_HIP_TRY(hipStreamSynchronize(stream));
  RGCN_HIP_TRY(hipMemcpyFromSymbol(host_flag, HIP_SYMBOL(g_index_error), sizeof(int)));
  RGCN_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_index_error), &zero, sizeof(int)));
  return RGCN_OK;
}

int distmult_fwd(const float* h, const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx,
                 int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows, int64_t batch, int64_t d,
                 float* scores, void* stream_) {
  return head_fwd_impl<DistMult, false>(h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows, nullptr, batch, d, scores,
                                        nullptr, (hipStream_t)stream_);
}

int distmult_bce_fwd(const float* h, const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx,
                     int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows, const float* labels,
                     int64_t batch, int64_t d, float* scores, float* loss, void* stream_) {
  return head_fwd_impl<DistMult, true>(h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows, labels, batch, d, scores,
                                       loss, (hipStream_t)stream_);
}

int distmult_bce_reduce(const float* loss, const float* scores, const float* labels, int64_t batch, float* mean_loss,
                        double* loss_sum, int64_t* correct, int64_t* cursor, int64_t cursor_add, void* stream_) {
  if (batch <= 0 || !loss || !mean_loss || (correct && (!scores || !labels))) return RGCN_ERR_ARG;
  if (batch > INT32_MAX / 2) return RGCN_ERR_UNSUPPORTED;
  RGCN_ALIGN_TRY(4, loss, scores, labels, mean_loss);
  RGCN_ALIGN_TRY(8, loss_sum, correct, cursor);
  k_bce_reduce<<<1, 1024, 0, (hipStream_t)stream_>>>(loss, scores, labels, (int)batch, mean_loss, loss_sum,
                                                     reinterpret_cast<long long*>(correct), reinterpret_cast<long long*>(cursor),
                                                     (long long)cursor_add);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

size_t distmult_bwd_workspace_bytes(int64_t batch, int64_t d, int64_t r_rows) {
  return head_bwd_workspace_bytes(batch, d, r_rows);
}

int distmult_bwd(const float* grad_scores, const float* h, const int64_t* h_idx, int64_t h_rows, const float* t,
                 const int64_t* t_idx, int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows,
                 int64_t batch, int64_t d, float* grad_h, float* grad_t, float* grad_r, void* workspace,
                 size_t workspace_bytes, int zero_tables, void* stream_) {
  return head_bwd_impl<DistMult, false>(grad_scores, nullptr, nullptr, h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows,
                                        batch, d, grad_h, grad_t, grad_r, workspace, workspace_bytes, zero_tables,
                                        (hipStream_t)stream_);
}

int distmult_bce_bwd(const float* grad_mean_loss, const float* scores, const float* labels, const float* h,
                     const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx, int64_t t_rows,
                     const float* r, const int64_t* r_idx, int64_t r_rows, int64_t batch, int64_t d, float* grad_h,
                     float* grad_t, float* grad_r, void* workspace, size_t workspace_bytes, int zero_tables,
                     void* stream_) {
  return head_bwd_impl<DistMult, true>(grad_mean_loss, scores, labels, h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows,
                                       batch, d, grad_h, grad_t, grad_r, workspace, workspace_bytes, zero_tables,
                                       (hipStream_t)stream_);
}

size_t rgcn_segment_sum_workspace_bytes(int64_t batch, int64_t d, int64_t num_rows) {
  if (batch <= 0 || d <= 0 || num_rows <= 0) return 0;
  return (size_t)ceil_div64(batch, segment_len(batch)) * num_rows * d * sizeof(float) + (size_t)batch * sizeof(int32_t) + 256;
}

int rgcn_segment_sum(const float* rows, const int64_t* idx, int64_t batch, int64_t d, int64_t num_rows, float* out,
                     void* workspace, size_t workspace_bytes, void* stream_) {
  if (batch < 0 || d <= 0 || (d & 3) || num_rows <= 0 || !out) return RGCN_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  if (batch == 0) {
    RGCN_HIP_TRY(hipMemsetAsync(out, 0, (size_t)num_rows * d * sizeof(float), stream));
    return RGCN_OK;
  }
  if (!rows || !idx) return RGCN_ERR_ARG;
  if (batch > INT32_MAX / 4 || num_rows > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < rgcn_segment_sum_workspace_bytes(batch, d, num_rows)) return RGCN_ERR_WORKSPACE;
  RGCN_ALIGN_TRY(16, rows, out, workspace);
  RGCN_ALIGN_TRY(8, idx);
  const int64_t nseg = ceil_div64(batch, segment_len(batch));
  float* partial = (float*)workspace;
  int32_t* keys = (int32_t*)(partial + (size_t)nseg * num_rows * d);
  k_keys32<<<(unsigned)ceil_div64(batch, 256), 256, 0, stream>>>(idx, batch, num_rows, keys);
  dim3 pg((unsigned)num_rows, (unsigned)nseg);
  k_segment_partials<<<pg, 64, 0, stream>>>(keys, (int)batch, rows, (int)d, (int)num_rows, (int)segment_len(batch), partial);
  k_segment_combine<false><<<(unsigned)num_rows, 64, 0, stream>>>(partial, (int)nseg, (int)num_rows, (int)d, out);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // extern "C"
