// ComplEx edge-scoring head (include/rgcn_complex.h): score(h, r, t) = Re <h, r, conj(t)>, asymmetric in h and t.
//
// A row of width d is m = d / 2 complex numbers, real parts in columns [0, m), imaginary parts in [m, d).  The kernels,
// the argument checks, the workspace layout and the deterministic backward are the decoder-head frame's
// (rgcn_decoder_head.h, shared with distmult.hip); this file is the ComplEx policy, the entry points that pick the
// frame's instances, and the query rows of the ranking passes (rgcn_complex_query).  One lane group of
// G = rgcn_pick_group(m) lanes per triple; a lane holds float4 column c of the real half and column c + m of the
// imaginary half of the head, relation and tail rows (six 16-byte loads per trip; the backward stores six).  The
// grouping of the products is the header's: the non-finite set of every output is float64's for that grouping.
#include "rgcn_common.h"
#include "rgcn_decoder_head.h"
#include "../../include/rgcn_complex.h"

namespace {

constexpr int kThreads = 256;                    // of the query launch

__device__ inline float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ inline float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ inline float4 scale4(float s, float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
__device__ inline void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// The policy of the frame - what a decoder must supply (rgcn_decoder_head.h has the list): the width multiple kWidth,
// the columns a lane group walks, one trip of the score and one trip of the three gradient rows.  Here: m = d / 2
// complex columns, the width a multiple of 8.
struct ComplEx {
  static constexpr int kWidth = 8;
  __host__ __device__ static inline int columns(int d) { return d >> 1; }
  __device__ static inline void score(const float* hp, const float* rp, const float* tp, int c, int d, float& s) {
    const int m = d >> 1;
    const float4 hre = ld4(hp + c), him = ld4(hp + m + c), rre = ld4(rp + c), rim = ld4(rp + m + c);
    const float4 tre = ld4(tp + c), tim = ld4(tp + m + c);
    const float4 qre = sub4(mul4(hre, rre), mul4(him, rim)), qim = add4(mul4(hre, rim), mul4(him, rre));
    s += qre.x * tre.x;
    s += qim.x * tim.x;
    s += qre.y * tre.y;
    s += qim.y * tim.y;
    s += qre.z * tre.z;
    s += qim.z * tim.z;
    s += qre.w * tre.w;
    s += qim.w * tim.w;
  }
  __device__ static inline void contrib(float g, const float* hp, const float* rp, const float* tp, int c, int d,
                                        float* out_h, float* out_t, float* out_r, size_t bo) {
    const int m = d >> 1;
    const float4 hre = ld4(hp + c), him = ld4(hp + m + c), rre = ld4(rp + c), rim = ld4(rp + m + c);
    const float4 tre = ld4(tp + c), tim = ld4(tp + m + c);
    if (out_h) {
      st4(out_h + bo + c, scale4(g, add4(mul4(rre, tre), mul4(rim, tim))));
      st4(out_h + bo + m + c, scale4(g, sub4(mul4(rre, tim), mul4(rim, tre))));
    }
    if (out_t) {
      st4(out_t + bo + c, scale4(g, sub4(mul4(hre, rre), mul4(him, rim))));
      st4(out_t + bo + m + c, scale4(g, add4(mul4(hre, rim), mul4(him, rre))));
    }
    if (out_r) {
      st4(out_r + bo + c, scale4(g, add4(mul4(hre, tre), mul4(him, tim))));
      st4(out_r + bo + m + c, scale4(g, sub4(mul4(hre, tim), mul4(him, tre))));
    }
  }
};

// q[b] = the rotation of x's row by rel's row (SIDE 0: tails of (x, rel, ?)) or by its conjugate (SIDE 1: heads of
// (?, rel, x)); one lane group per query row
template <int G>
__global__ __launch_bounds__(kThreads) void k_complex_query(int side, const float* __restrict__ x,
                                                            const int64_t* __restrict__ xi, int64_t x_rows,
                                                            const float* __restrict__ r, const int64_t* __restrict__ ri,
                                                            int64_t r_rows, int64_t B, int d, float* __restrict__ q,
                                                            int* __restrict__ flag) {
  const int64_t b = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / G;
  const int gl = threadIdx.x % G;
  if (b >= B) return;
  const int m = d >> 1;
  const float* xp = x + (size_t)rgcn_checked_row(xi, b, x_rows, flag) * d;
  const float* rp = r + (size_t)rgcn_checked_row(ri, b, r_rows, flag) * d;
  float* qp = q + (size_t)b * d;
  for (int c = gl * 4; c < m; c += G * 4) {
    const float4 xre = ld4(xp + c), xim = ld4(xp + m + c), rre = ld4(rp + c), rim = ld4(rp + m + c);
    if (side == 0) {
      st4(qp + c, sub4(mul4(xre, rre), mul4(xim, rim)));
      st4(qp + m + c, add4(mul4(xre, rim), mul4(xim, rre)));
    } else {
      st4(qp + c, add4(mul4(rre, xre), mul4(rim, xim)));
      st4(qp + m + c, sub4(mul4(rre, xim), mul4(rim, xre)));
    }
  }
}

}  // namespace

extern "C" {

int complex_fwd(const float* h, const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx,
                int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows, int64_t batch, int64_t d,
                float* scores, void* stream_) {
  return head_fwd_impl<ComplEx, false>(h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows, nullptr, batch, d, scores,
                                       nullptr, (hipStream_t)stream_);
}

int complex_bce_fwd(const float* h, const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx,
                    int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows, const float* labels,
                    int64_t batch, int64_t d, float* scores, float* loss, void* stream_) {
  return head_fwd_impl<ComplEx, true>(h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows, labels, batch, d, scores, loss,
                                      (hipStream_t)stream_);
}

size_t complex_bwd_workspace_bytes(int64_t batch, int64_t d, int64_t r_rows) {
  return head_bwd_workspace_bytes(batch, d, r_rows);
}

int complex_bwd(const float* grad_scores, const float* h, const int64_t* h_idx, int64_t h_rows, const float* t,
                const int64_t* t_idx, int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows,
                int64_t batch, int64_t d, float* grad_h, float* grad_t, float* grad_r, void* workspace,
                size_t workspace_bytes, int zero_tables, void* stream_) {
  return head_bwd_impl<ComplEx, false>(grad_scores, nullptr, nullptr, h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows,
                                       batch, d, grad_h, grad_t, grad_r, workspace, workspace_bytes, zero_tables,
                                       (hipStream_t)stream_);
}

int complex_bce_bwd(const float* grad_mean_loss, const float* scores, const float* labels, const float* h,
                    const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx, int64_t t_rows,
                    const float* r, const int64_t* r_idx, int64_t r_rows, int64_t batch, int64_t d, float* grad_h,
                    float* grad_t, float* grad_r, void* workspace, size_t workspace_bytes, int zero_tables,
                    void* stream_) {
  return head_bwd_impl<ComplEx, true>(grad_mean_loss, scores, labels, h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows,
                                      batch, d, grad_h, grad_t, grad_r, workspace, workspace_bytes, zero_tables,
                                      (hipStream_t)stream_);
}

int rgcn_complex_query(int side, const float* x, const int64_t* x_idx, int64_t x_rows, const float* rel,
                       const int64_t* rel_idx, int64_t rel_rows, int64_t batch, int64_t d, float* q, void* stream_) {
  if ((side != 0 && side != 1) || batch < 0 || d <= 0 || (d & 7) || x_rows < 0 || rel_rows < 0) return RGCN_ERR_ARG;
  if (batch == 0) return RGCN_OK;
  if (!x || !rel || !q) return RGCN_ERR_ARG;
  if (d > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  RGCN_ALIGN_TRY(16, x, rel, q);
  RGCN_ALIGN_TRY(8, x_idx, rel_idx);
  int* flag = rgcn_index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  const int g = rgcn_pick_group(d / 2);
  const unsigned grid = (unsigned)ceil_div64(batch, kThreads / g);
  RGCN_DISPATCH_G(g, (k_complex_query<G><<<grid, kThreads, 0, (hipStream_t)stream_>>>(side, x, x_idx, x_rows, rel, rel_idx,
                                                                                    rel_rows, batch, (int)d, q, flag)));
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // extern "C"
