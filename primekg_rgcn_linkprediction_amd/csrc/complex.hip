// ComplEx edge-scoring head (include/rgcn_complex.h): score(h, r, t) = Re <h, r, conj(t)>, asymmetric in h and t.
//
// A row of width d is m = d / 2 complex numbers, real parts in columns [0, m), imaginary parts in [m, d).  One lane group
// of G = rgcn_pick_group(m) lanes per triple; a lane holds float4 column c of the real half and column c + m of the
// imaginary half of the head, relation and tail rows (six 16-byte loads), wavefront butterfly (__shfl_xor) reduction
// over the group - no LDS, no intermediate [B, d] tensors.  The grouping of the products is the header's: the
// non-finite set of every output is float64's for that grouping.
//
// The backward is the DistMult head's (distmult.hip), deterministic, with another first launch:
//   1. k_complex_contrib: per sample the three gradient rows, six 16-byte stores per lane and trip - into the caller's
//      buffer for an operand without an index, otherwise into workspace rows - the sample's row ids as int32 keys, and
//      the rider workgroups that clear the gradient tables (zero_tables).
//   2. k_scatter_rows and 3. k_segment_partials / k_segment_combine: decoder-independent, from rgcn_ordered_match.h.
#include "rgcn_common.h"
#include "rgcn_ordered_match.h"
#include "../../include/rgcn_complex.h"

namespace {

constexpr int kThreads = 256;

// binary_cross_entropy_with_logits per element, the way aten evaluates it (distmult.hip)
__device__ inline float bce_with_logits(float x, float y) {
  return (1.f - y) * x - (fminf(x, 0.f) - log1pf(expf(-fabsf(x))));
}

__device__ inline float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ inline float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ inline float4 scale4(float s, float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, s * a.w); }
__device__ inline void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

template <int G, bool BCE = false>
__global__ __launch_bounds__(kThreads) void k_complex_fwd(const float* __restrict__ h, const int64_t* __restrict__ hi,
                                                          int64_t h_rows, const float* __restrict__ t,
                                                          const int64_t* __restrict__ ti, int64_t t_rows,
                                                          const float* __restrict__ r, const int64_t* __restrict__ ri,
                                                          int64_t r_rows, int64_t B, int d, float* __restrict__ scores,
                                                          int* __restrict__ flag, const float* __restrict__ labels = nullptr,
                                                          float* __restrict__ loss = nullptr) {
  const int64_t b = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / G;
  const int gl = threadIdx.x % G;
  const bool live = b < B;                       // lanes past the batch stay for the butterfly
  const int m = d >> 1;
  float s = 0.f;
  if (live) {
    const float* hp = h + (size_t)rgcn_checked_row(hi, b, h_rows, flag) * d;
    const float* tp = t + (size_t)rgcn_checked_row(ti, b, t_rows, flag) * d;
    const float* rp = r + (size_t)rgcn_checked_row(ri, b, r_rows, flag) * d;
    for (int c = gl * 4; c < m; c += G * 4) {
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
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, G);
  if (live && gl == 0) {
    scores[b] = s;
    if (BCE) loss[b] = bce_with_logits(s, labels[b]);
  }
}

template <int G, bool BCE = false>
__global__ __launch_bounds__(kThreads) void k_complex_contrib(
    const float* __restrict__ gs, const float* __restrict__ h, const int64_t* __restrict__ hi, int64_t h_rows,
    const float* __restrict__ t, const int64_t* __restrict__ ti, int64_t t_rows, const float* __restrict__ r,
    const int64_t* __restrict__ ri, int64_t r_rows, int64_t B, int d, float* __restrict__ out_h,
    float* __restrict__ out_t, float* __restrict__ out_r, int32_t* __restrict__ key_h, int32_t* __restrict__ key_t,
    int32_t* __restrict__ key_r, const float* __restrict__ scores, const float* __restrict__ labels, int work_blocks,
    float* __restrict__ zero_a, int64_t zero_a_quads, float* __restrict__ zero_b, int64_t zero_b_quads,
    int* __restrict__ flag) {
  if ((int)blockIdx.x >= work_blocks) {          // riders: zero the gradient tables the scatter launch writes rows into
    const int64_t stride = (int64_t)(gridDim.x - work_blocks) * kThreads;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t q = (int64_t)((int)blockIdx.x - work_blocks) * kThreads + threadIdx.x; q < zero_a_quads + zero_b_quads; q += stride) {
      if (q < zero_a_quads) reinterpret_cast<float4*>(zero_a)[q] = z;
      else reinterpret_cast<float4*>(zero_b)[q - zero_a_quads] = z;
    }
    return;
  }
  const int64_t b = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / G;
  const int gl = threadIdx.x % G;
  if (b >= B) return;
  const int64_t hr = rgcn_checked_row(hi, b, h_rows, flag), tr = rgcn_checked_row(ti, b, t_rows, flag),
                rr = rgcn_checked_row(ri, b, r_rows, flag);
  if (gl == 0) {
    if (key_h) key_h[b] = (int32_t)hr;
    if (key_t) key_t[b] = (int32_t)tr;
    if (key_r) key_r[b] = (int32_t)rr;
  }
  const int m = d >> 1;
  const size_t ho = (size_t)hr * d, to = (size_t)tr * d, ro = (size_t)rr * d, bo = (size_t)b * d;
  const float g = BCE ? gs[0] * (1.f / (1.f + expf(-scores[b])) - labels[b]) / (float)B : gs[b];
  for (int c = gl * 4; c < m; c += G * 4) {
    const float4 hre = ld4(h + ho + c), him = ld4(h + ho + m + c), rre = ld4(r + ro + c), rim = ld4(r + ro + m + c);
    const float4 tre = ld4(t + to + c), tim = ld4(t + to + m + c);
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
}

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

// the sticky index-error flag of the current device, looked up once per device: the lookup is not a stream operation,
// so a call that is being captured into a HIP graph must not make it (an eager call comes first)
int* index_error_flag() {
  static int* flags[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  if (dev < 0 || dev >= 64) return rgcn_index_error_flag();
  if (!flags[dev]) flags[dev] = rgcn_index_error_flag();
  return flags[dev];
}

// the shared body of complex_fwd / complex_bce_fwd
template <bool BCE>
int fwd_impl(const float* h, const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx, int64_t t_rows,
             const float* r, const int64_t* r_idx, int64_t r_rows, const float* labels, int64_t batch, int64_t d,
             float* scores, float* loss, hipStream_t stream) {
  if (batch < 0 || d <= 0 || (d & 7) || h_rows < 0 || t_rows < 0 || r_rows < 0) return RGCN_ERR_ARG;
  if (batch == 0) return RGCN_OK;
  if (!h || !t || !r || !scores || (BCE && (!labels || !loss))) return RGCN_ERR_ARG;
  if (d > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  RGCN_ALIGN_TRY(16, h, t, r);
  RGCN_ALIGN_TRY(8, h_idx, t_idx, r_idx);
  RGCN_ALIGN_TRY(4, labels, scores, loss);
  int* flag = index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  const int g = rgcn_pick_group(d / 2);
  const unsigned grid = (unsigned)ceil_div64(batch, kThreads / g);
  RGCN_DISPATCH_G(g, (k_complex_fwd<G, BCE><<<grid, kThreads, 0, stream>>>(h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows,
                                                                        batch, (int)d, scores, flag, labels, loss)));
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

// the shared body of complex_bwd / complex_bce_bwd: distmult.hip's, with this file's first launch
template <bool BCE>
int bwd_impl(const float* gs, const float* scores, const float* labels, const float* h, const int64_t* h_idx,
             int64_t h_rows, const float* t, const int64_t* t_idx, int64_t t_rows, const float* r, const int64_t* r_idx,
             int64_t r_rows, int64_t batch, int64_t d, float* grad_h, float* grad_t, float* grad_r, void* workspace,
             size_t workspace_bytes, int zero_tables, hipStream_t stream) {
  if (batch < 0 || d <= 0 || (d & 7) || h_rows < 0 || t_rows < 0 || r_rows < 0) return RGCN_ERR_ARG;
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
  if (!gs || !h || !t || !r) return RGCN_ERR_ARG;
  if (batch > INT32_MAX / 4 || h_rows > INT32_MAX || t_rows > INT32_MAX || r_rows > INT32_MAX || d > INT32_MAX)
    return RGCN_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < complex_bwd_workspace_bytes(batch, d, r_idx ? r_rows : 0)) return RGCN_ERR_WORKSPACE;
  RGCN_ALIGN_TRY(16, h, t, r, grad_h, grad_t, grad_r, workspace);
  RGCN_ALIGN_TRY(8, h_idx, t_idx, r_idx);
  RGCN_ALIGN_TRY(4, gs, scores, labels);
  int* flag = index_error_flag();
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
  const int g = rgcn_pick_group(d / 2);
  const unsigned grid = (unsigned)ceil_div64(batch, kThreads / g);
  const bool sh = grad_h && h_idx, st = grad_t && t_idx;
  // zero_tables: the tables the scatter below writes rows into are cleared by riders of this launch (the relation
  // table is written whole by its tree)
  float *za = nullptr, *zb = nullptr;
  int64_t zaq = 0, zbq = 0;
  if (zero_tables) {
    if (sh) { za = grad_h; zaq = h_rows * d / 4; }
    if (st && !(sh && grad_h == grad_t)) { zb = grad_t; zbq = t_rows * d / 4; }
  }
  const unsigned riders = (zaq + zbq) > 0 ? (unsigned)std::min<int64_t>(1024, ceil_div64(zaq + zbq, 4 * kThreads)) : 0u;
  RGCN_DISPATCH_G(g, (k_complex_contrib<G, BCE><<<grid + riders, kThreads, 0, stream>>>(
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

extern "C" {

int complex_fwd(const float* h, const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx,
                int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows, int64_t batch, int64_t d,
                float* scores, void* stream_) {
  return fwd_impl<false>(h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows, nullptr, batch, d, scores, nullptr,
                         (hipStream_t)stream_);
}

int complex_bce_fwd(const float* h, const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx,
                    int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows, const float* labels,
                    int64_t batch, int64_t d, float* scores, float* loss, void* stream_) {
  return fwd_impl<true>(h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows, labels, batch, d, scores, loss,
                        (hipStream_t)stream_);
}

size_t complex_bwd_workspace_bytes(int64_t batch, int64_t d, int64_t r_rows) {
  if (batch <= 0 || d <= 0) return 0;
  const int64_t nseg = ceil_div64(batch, segment_len(batch));
  return ((size_t)3 * batch * d + (size_t)nseg * (r_rows > 0 ? r_rows : 0) * d) * sizeof(float) +
         (size_t)3 * batch * sizeof(int32_t) + 256;
}

int complex_bwd(const float* grad_scores, const float* h, const int64_t* h_idx, int64_t h_rows, const float* t,
                const int64_t* t_idx, int64_t t_rows, const float* r, const int64_t* r_idx, int64_t r_rows,
                int64_t batch, int64_t d, float* grad_h, float* grad_t, float* grad_r, void* workspace,
                size_t workspace_bytes, int zero_tables, void* stream_) {
  return bwd_impl<false>(grad_scores, nullptr, nullptr, h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows, batch, d,
                         grad_h, grad_t, grad_r, workspace, workspace_bytes, zero_tables, (hipStream_t)stream_);
}

int complex_bce_bwd(const float* grad_mean_loss, const float* scores, const float* labels, const float* h,
                    const int64_t* h_idx, int64_t h_rows, const float* t, const int64_t* t_idx, int64_t t_rows,
                    const float* r, const int64_t* r_idx, int64_t r_rows, int64_t batch, int64_t d, float* grad_h,
                    float* grad_t, float* grad_r, void* workspace, size_t workspace_bytes, int zero_tables,
                    void* stream_) {
  if (batch > 0 && (!scores || !labels)) return RGCN_ERR_ARG;
  return bwd_impl<true>(grad_mean_loss, scores, labels, h, h_idx, h_rows, t, t_idx, t_rows, r, r_idx, r_rows, batch, d,
                        grad_h, grad_t, grad_r, workspace, workspace_bytes, zero_tables, (hipStream_t)stream_);
}

int rgcn_complex_query(int side, const float* x, const int64_t* x_idx, int64_t x_rows, const float* rel,
                       const int64_t* rel_idx, int64_t rel_rows, int64_t batch, int64_t d, float* q, void* stream_) {
  if ((side != 0 && side != 1) || batch < 0 || d <= 0 || (d & 7) || x_rows < 0 || rel_rows < 0) return RGCN_ERR_ARG;
  if (batch == 0) return RGCN_OK;
  if (!x || !rel || !q) return RGCN_ERR_ARG;
  if (d > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  RGCN_ALIGN_TRY(16, x, rel, q);
  RGCN_ALIGN_TRY(8, x_idx, rel_idx);
  int* flag = index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  const int g = rgcn_pick_group(d / 2);
  const unsigned grid = (unsigned)ceil_div64(batch, kThreads / g);
  RGCN_DISPATCH_G(g, (k_complex_query<G><<<grid, kThreads, 0, (hipStream_t)stream_>>>(side, x, x_idx, x_rows, rel, rel_idx,
                                                                                    rel_rows, batch, (int)d, q, flag)));
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // extern "C"
