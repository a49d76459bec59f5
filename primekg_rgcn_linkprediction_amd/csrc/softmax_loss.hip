// 1-vs-all softmax cross-entropy of the true entity against every candidate, and its gradients, without the [B, N]
// score matrix (include/rgcn_softmax.h: contract, grouping, order of every sum).
//
//   score[b, n] = <q[b], emb[n]>   - the k-tile of rgcn_mma_f32_dma.h: the bits distmult_score_all_tails stores and
//                                    k_rank_count / k_topk_select compare
//
// Forward, grid (ceil(B / 64), S): mma_f32_dma::walk_tiles over the slice's 128-column tiles exactly as k_topk_select
// uses it - the mask words are its `pre`, the log-sum-exp its `epi`.  A lane keeps a running (m, sum) for each of its
// 16 rows over the columns it sees (its own column of the wave's two 32-column groups, every tile), so the epilogue is
// lane-local: no cross-lane traffic but the mask words.  After the walk the 32 lanes of a row merge by a butterfly, the
// two wave columns through LDS, and k_softmax_merge the slices in slice order.
// Backward, ONE kernel template, two instantiations (DE = false: dq, a workgroup owns 64 query rows and streams
// candidate tiles of a slice; DE = true: dE, a workgroup owns 64 candidate rows and streams all query tiles).  Per
// streamed tile: the walk recomputes the score tile, `epi` forms the coefficient tile from lse and the masks (read
// transposed for dE), puts it into LDS, and multiplies it - the A operand, read back in the k-tile's own fragment order -
// with the streamed rows themselves (B_KN form: rows as they lie in memory, fetched through the cache the DMA of the
// score pass has just filled) into an output tile of 64 x d that lives in accumulators for the whole walk.
#include <math.h>

#include "rgcn_candidate_filter.h"    // and with it rgcn_common.h and rgcn_mma_f32_dma.h
#include "../../include/rgcn_softmax.h"

namespace {

using namespace mma_f32_dma;    // kThreads (256: 4 waves, 2 (m) x 2 (n)), BK, BM, NBUF, walk_tiles, acc_row, the vector types

typedef KTile<2, B_BLK> Tile;   // 64 x 128 scores per workgroup
constexpr int BN = Tile::BN, BUF_FLOATS = Tile::BUF_FLOATS;
constexpr int RING_FLOATS = NBUF * BUF_FLOATS;                   // 73,728 B; the ring is the first LDS object
constexpr int LDC = BN + 4;                                      // row pitch of the coefficient tile (floats; 16-byte rows)
constexpr int kMaxSlices = 64;
constexpr int kMaxD = 256;

constexpr size_t kFwdLds = (size_t)(RING_FLOATS + 2 * BM) * 4;
constexpr size_t kBwdLds = (size_t)(RING_FLOATS + BM * LDC) * 4;  // 107,520 B: one workgroup per CU

// max that keeps a NaN (fmaxf drops it): the maximum of the contract is float64's, which does not
__device__ inline float nan_max(float a, float b) {
  const float m = fmaxf(a, b);
  return a != a ? a : (b != b ? b : m);
}
// the factor that carries a sum kept relative to `from` over to `to` (to >= from): exactly 1 on the side that holds the
// maximum, so two -inf (nothing eligible yet) never meet in a subtraction
__device__ inline float rescale(float from, float to) { return from == to ? 1.f : expf(from - to); }
// an eligible score's term relative to m; -inf (an ineligible candidate is handed over as -inf) is an exact zero
__device__ inline float lse_term(float x, float m) { return x == -INFINITY ? 0.f : expf(x - m); }
// (m, l) <- merge of (m, l) and (m2, l2).  No contraction: the butterfly needs a + b == b + a bit for bit.
__device__ inline void lse_merge(float& m, float& l, float m2, float l2) {
  const float mn = nan_max(m, m2);
  l = __fadd_rn(__fmul_rn(l, rescale(m, mn)), __fmul_rn(l2, rescale(m2, mn)));
  m = mn;
}

__device__ inline int checked_target(const int64_t* __restrict__ target, int b, int N, int* __restrict__ flag) {
  const int64_t v = target[b];
  if ((uint64_t)v >= (uint64_t)N) {
    *flag = 1;
    return 0;
  }
  return (int)v;
}

__global__ __launch_bounds__(kThreads) void k_softmax_fwd(const float* __restrict__ q, const float* __restrict__ emb,
                                                          const int64_t* __restrict__ target,
                                                          const uint32_t* __restrict__ allow,
                                                          const int32_t* __restrict__ qcls, int num_classes,
                                                          const uint32_t* __restrict__ excl, int M, int N, int d,
                                                          int tiles_per_slice, int num_tiles, float* __restrict__ ws_m,
                                                          float* __restrict__ ws_l, float* __restrict__ true_score,
                                                          int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* s_m = lds + RING_FLOATS;
  float* s_l = s_m + BM;

  const int m0 = blockIdx.x * BM;
  const int ct_begin = blockIdx.y * tiles_per_slice, ct_end = min(num_tiles, ct_begin + tiles_per_slice);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int words = (N + 31) >> 5;

  // this lane's mask row: lanes 0-31 carry the first 32-column group of the wave, lanes 32-63 the second
  lane_filter filt(allow, qcls, num_classes, excl, m0 + wm * 32 + li, M, words);

  int tg[16];                                                    // the targets of this lane's 16 rows
  float rm[16], rl[16];                                          // their running (max, sum relative to it)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    tg[r] = checked_target(target, min(m0 + wm * 32 + acc_row(r, lh), M - 1), N, flag);
    rm[r] = -INFINITY;
    rl[r] = 0.f;
  }

  Tile tile(wm, wn, li, lh);
  auto pre = [&](int ct) { filt.load(ct * BN + (wn * 2 + lh) * 32); };
  auto epi = [&](int ct, floatx16 (&acc)[2]) {
    const unsigned okw = filt.word();
    const int c0 = ct * BN + wn * 64 + li, c1 = c0 + 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rowl = acc_row(r, lh);
      const unsigned w0 = (unsigned)__shfl((int)okw, rowl), w1 = (unsigned)__shfl((int)okw, 32 + rowl);
      const bool t0 = c0 == tg[r], t1 = c1 == tg[r];             // (a target is inside [0, N))
      const bool e0 = (c0 < N && ((w0 >> li) & 1u)) || t0, e1 = (c1 < N && ((w1 >> li) & 1u)) || t1;
      const float v0 = acc[0][r], v1 = acc[1][r];
      if (t0 || t1) {
        const int row = m0 + wm * 32 + rowl;
        if (row < M) true_score[row] = t0 ? v0 : v1;
      }
      const float x0 = e0 ? v0 : -INFINITY, x1 = e1 ? v1 : -INFINITY;
      const float mn = nan_max(rm[r], nan_max(x0, x1));
      rl[r] = rl[r] * rescale(rm[r], mn) + (lse_term(x0, mn) + lse_term(x1, mn));
      rm[r] = mn;
    }
  };
  // rows past M and columns past N read a valid row; never eligible / never written
  walk_tiles(lds, q, emb, M, d, m0, ct_begin, ct_end, wave, lane, tile, [&](int n) { return min(n, N - 1); }, pre, epi);

  // the 32 chains of a row (lane distance 1 .. 16 stays inside the half), then wave column 0 with wave column 1
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
      const float m2 = __shfl_xor(rm[r], o), l2 = __shfl_xor(rl[r], o);
      lse_merge(rm[r], rl[r], m2, l2);
    }
  }
  __syncthreads();
  if (wn == 1 && li == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s_m[wm * 32 + acc_row(r, lh)] = rm[r];
      s_l[wm * 32 + acc_row(r, lh)] = rl[r];
    }
  }
  __syncthreads();
  if (wn == 0 && li == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rowl = wm * 32 + acc_row(r, lh), row = m0 + rowl;
      lse_merge(rm[r], rl[r], s_m[rowl], s_l[rowl]);
      if (row < M) {
        ws_m[(size_t)blockIdx.y * M + row] = rm[r];
        ws_l[(size_t)blockIdx.y * M + row] = rl[r];
      }
    }
  }
}

// The slices of a row in slice order; lse, the row's maximum and, when asked for, loss and hit.  One thread per row and
// S steps: this runs in float64 and lse is rounded ONCE.  logf is good to 1 ulp, but its error is a smooth function of
// its argument: on an untrained model every row's sum is nearly the same number, every lse was off to the same side
// (about 1e-7), sum_n c[b, n] had the same sign in every row, and the gradients of the encoder's parameters, which add
// the rows up, were ten times as far from float64 as a float32 CPU run's.
__device__ inline double nan_max64(double a, double b) { return a != a ? a : (b != b ? b : fmax(a, b)); }
__device__ inline double rescale64(double from, double to) { return from == to ? 1.0 : exp(from - to); }
__global__ __launch_bounds__(kThreads) void k_softmax_merge(const float* __restrict__ ws_m, const float* __restrict__ ws_l,
                                                            const float* __restrict__ true_score, int M, int S,
                                                            float* __restrict__ lse, float* __restrict__ row_max,
                                                            float* __restrict__ loss, int32_t* __restrict__ hit) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= M) return;
  double m = ws_m[b], l = ws_l[b];
  for (int s = 1; s < S; ++s) {
    const double m2 = ws_m[(size_t)s * M + b], l2 = ws_l[(size_t)s * M + b];
    const double mn = nan_max64(m, m2);
    l = l * rescale64(m, mn) + l2 * rescale64(m2, mn);
    m = mn;
  }
  const float v = (float)(m + log(l));
  const float mf = (float)m;                                     // exact: the maximum is one of the fp32 scores
  lse[b] = v;
  row_max[b] = mf;
  const float ts = true_score[b];
  if (loss) loss[b] = v - ts;
  if (hit) hit[b] = ts >= mf ? 1 : 0;
}

// NB: 32-column blocks of the output tile a wave owns (wave column wn: blocks wn * NB .. wn * NB + NB - 1 of d / 32).
// own [M_own, d]: the rows the workgroup owns; str [N_str, d]: the rows it streams.  N candidates, Bq queries.
template <int NB, bool DE>
__global__ __launch_bounds__(kThreads) void k_softmax_bwd(const float* __restrict__ g, const float* __restrict__ own,
                                                          const float* __restrict__ str,
                                                          const int64_t* __restrict__ target,
                                                          const uint32_t* __restrict__ allow,
                                                          const int32_t* __restrict__ qcls, int num_classes,
                                                          const uint32_t* __restrict__ excl,
                                                          const float* __restrict__ lse, int Bq, int N, int d,
                                                          int tiles_per_slice, int num_tiles, float* __restrict__ dst,
                                                          size_t slab_floats, int accumulate, int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* s_c = lds + RING_FLOATS;                                // the coefficient tile [64][LDC]

  const int M_own = DE ? N : Bq, N_str = DE ? Bq : N;
  const int m0 = blockIdx.x * BM;
  const int ct_begin = blockIdx.y * tiles_per_slice, ct_end = min(num_tiles, ct_begin + tiles_per_slice);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int words = (N + 31) >> 5;
  const int nblk = d >> 5;

  floatx16 out[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[j][r] = 0.f;

  // dq: per ROW (query) quantities of this lane's 16 rows, and the mask words as the forward carries them.
  // dE: per COLUMN (query) quantities of this lane's two columns, loaded tile by tile in `pre`; the mask word of a
  //     query over the wave's 32 candidate rows is one word, (m0 + wm * 32) >> 5 - the mask read transposed.
  int tg[DE ? 2 : 16];
  float gl[DE ? 2 : 16], ls[DE ? 2 : 16];
  unsigned okc[2] = {0u, 0u};
  lane_filter filt;
  if constexpr (!DE) {
    filt = lane_filter(allow, qcls, num_classes, excl, m0 + wm * 32 + li, Bq, words);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = min(m0 + wm * 32 + acc_row(r, lh), Bq - 1);
      tg[r] = checked_target(target, row, N, flag);
      gl[r] = g[row];
      ls[r] = lse[row];
    }
  }
  const int w_own = min((m0 + wm * 32) >> 5, words - 1);          // dE: the word of the wave's 32 candidate rows

  Tile tile(wm, wn, li, lh);
  auto pre = [&](int ct) {
    if constexpr (!DE) {
      filt.load(ct * BN + (wn * 2 + lh) * 32);
    } else {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int bq = min(ct * BN + (wn * 2 + b) * 32 + li, Bq - 1);
        tg[b] = checked_target(target, bq, N, flag);
        gl[b] = g[bq];
        ls[b] = lse[bq];
        unsigned aw = 0xffffffffu, ew = 0u;
        if (allow) {
          const int c = qcls[bq];
          const bool ok = c >= 0 && c < num_classes;
          aw = allow[(size_t)(ok ? c : 0) * words + w_own];
          aw = ok ? aw : 0u;
        }
        if (excl) ew = excl[(size_t)bq * words + w_own];
        okc[b] = aw & ~ew;
      }
    }
  };
  auto epi = [&](int ct, floatx16 (&acc)[2]) {
    // the coefficient tile -> LDS.  An ineligible entry is an exact 0 (selected), a streamed column past the end too.
    const unsigned okw = filt.word();                             // (dq)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rowl = acc_row(r, lh);
      unsigned w[2] = {0u, 0u};
      if constexpr (!DE) {
        w[0] = (unsigned)__shfl((int)okw, rowl);
        w[1] = (unsigned)__shfl((int)okw, 32 + rowl);
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int col = ct * BN + (wn * 2 + b) * 32 + li;        // streamed index: a candidate (dq) or a query (dE)
        const float v = acc[b][r];
        bool tgt, bit;
        float gg, ll;
        if constexpr (!DE) {
          tgt = col == tg[r];
          bit = (w[b] >> li) & 1u;
          gg = gl[r];
          ll = ls[r];
        } else {
          tgt = m0 + wm * 32 + rowl == tg[b];
          bit = (okc[b] >> rowl) & 1u;
          gg = gl[b];
          ll = ls[b];
        }
        const bool valid = col < N_str;
        const float p = (bit || tgt) ? expf(v - ll) : 0.f;
        const float c = valid ? gg * (p - (tgt ? 1.f : 0.f)) : 0.f;
        s_c[(wm * 32 + rowl) * LDC + (wn * 2 + b) * 32 + li] = c;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // out[32 rows of the wave][NB blocks] += c[32 rows][128] x str[128 streamed rows][NB blocks]; k in the fragment
    // order of the shared tile: a step of 8 streamed rows, lane half lh takes rows 8 s + 4 lh .. + 3
    const float* crow = s_c + (wm * 32 + li) * LDC + 4 * lh;
    const int nbase = ct * BN + 4 * lh;
#pragma unroll 2
    for (int s8 = 0; s8 < BN / 8; ++s8) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(crow + 8 * s8);
      const float* r0 = str + (size_t)min(nbase + 8 * s8 + 0, N_str - 1) * d + li;
      const float* r1 = str + (size_t)min(nbase + 8 * s8 + 1, N_str - 1) * d + li;
      const float* r2 = str + (size_t)min(nbase + 8 * s8 + 2, N_str - 1) * d + li;
      const float* r3 = str + (size_t)min(nbase + 8 * s8 + 3, N_str - 1) * d + li;
      float fb[NB][4];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int blk = wn * NB + j;
        if (blk < nblk) {                                        // wave-uniform
          fb[j][0] = r0[blk * 32];
          fb[j][1] = r1[blk * 32];
          fb[j][2] = r2[blk * 32];
          fb[j][3] = r3[blk * 32];
        }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (wn * NB + j < nblk) {
          out[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, fb[j][0], out[j], 0, 0, 0);
          out[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, fb[j][1], out[j], 0, 0, 0);
          out[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, fb[j][2], out[j], 0, 0, 0);
          out[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, fb[j][3], out[j], 0, 0, 0);
        }
      }
    }
    // (the next tile's coefficients are written behind at least one barrier of the walk: every wave is done reading)
  };
  walk_tiles(lds, own, str, M_own, d, m0, ct_begin, ct_end, wave, lane, tile, [&](int n) { return min(n, N_str - 1); }, pre,
             epi);

  float* o = dst + (size_t)blockIdx.y * slab_floats;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int blk = wn * NB + j;
    if (blk < nblk) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 + acc_row(r, lh);
        if (row < M_own) {
          float* p = o + (size_t)row * d + blk * 32 + li;
          *p = accumulate ? *p + out[j][r] : out[j][r];
        }
      }
    }
  }
}

// dq = slab 0 + slab 1 + ... in slice order, four floats per thread
__global__ __launch_bounds__(kThreads) void k_softmax_slab_sum(const float* __restrict__ slabs, size_t slab_floats, int S,
                                                               float* __restrict__ dq) {
  const size_t i = ((size_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (i >= slab_floats) return;
  f32x4 v = *reinterpret_cast<const f32x4*>(slabs + i);
  for (int s = 1; s < S; ++s) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(slabs + (size_t)s * slab_floats + i);
    v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
  }
  *reinterpret_cast<f32x4*>(dq + i) = v;
}

// the checks both entry points share, in the header's order
inline int check_shape(int64_t batch, int64_t num_entities, int64_t d, int64_t slices, int64_t num_classes,
                       const uint32_t* allow, const int32_t* query_class) {
  if (batch < 0 || num_entities <= 0 || d <= 0 || slices < 0) return RGCN_ERR_ARG;
  if ((d % BK) || d > kMaxD) return RGCN_ERR_UNSUPPORTED;
  if (!filter_args_ok(allow, query_class, num_classes)) return RGCN_ERR_ARG;
  return RGCN_OK;
}

template <bool DE>
int launch_bwd(int nb, dim3 grid, hipStream_t stream, const float* g, const float* own, const float* str,
               const int64_t* target, const uint32_t* allow, const int32_t* qcls, int num_classes, const uint32_t* excl,
               const float* lse, int Bq, int N, int d, int tiles_per_slice, int num_tiles, float* dst, size_t slab_floats,
               int accumulate, int* flag) {
  static bool raised[4][64] = {};
#define SOFTMAX_BWD_CASE(NB_)                                                                                       \
  case NB_: {                                                                                                       \
    const int rc = raise_lds(k_softmax_bwd<NB_, DE>, (int)kBwdLds, raised[NB_ - 1]);                                \
    if (rc) return rc;                                                                                              \
    k_softmax_bwd<NB_, DE><<<grid, kThreads, kBwdLds, stream>>>(g, own, str, target, allow, qcls, num_classes, excl, \
                                                                lse, Bq, N, d, tiles_per_slice, num_tiles, dst,     \
                                                                slab_floats, accumulate, flag);                     \
  } break;
  switch (nb) {
    SOFTMAX_BWD_CASE(1)
    SOFTMAX_BWD_CASE(2)
    SOFTMAX_BWD_CASE(3)
    default:
    SOFTMAX_BWD_CASE(4)
  }
#undef SOFTMAX_BWD_CASE
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace

extern "C" {

size_t rgcn_softmax_workspace_bytes(int64_t batch, int64_t num_entities, int64_t d, int64_t slices) {
  if (batch <= 0 || num_entities <= 0 || d <= 0 || slices < 0) return 0;
  const entity_slices p = plan_entity_slices(batch, num_entities, slices, kMaxSlices);
  const size_t fwd = (size_t)2 * p.slices * batch * sizeof(float);                       // (m, sum) per slice and row
  const size_t bwd = p.slices > 1 ? (size_t)p.slices * batch * d * sizeof(float) : 0;    // the partial dq slabs
  return align256(fwd > bwd ? fwd : bwd);
}

int rgcn_softmax_lse(const float* q, const float* emb, const int64_t* target, const uint32_t* allow,
                     const int32_t* query_class, int64_t num_classes, const uint32_t* exclude, int64_t batch,
                     int64_t num_entities, int64_t d, int64_t slices, float* lse, float* true_score, float* row_max,
                     float* loss, int32_t* hit, void* workspace, size_t workspace_bytes, void* stream_) {
  const int bad = check_shape(batch, num_entities, d, slices, num_classes, allow, query_class);
  if (bad) return bad;
  if (batch == 0) return RGCN_OK;
  if (!q || !emb || !target || !lse || !true_score || !row_max) return RGCN_ERR_ARG;
  if (!candidate_range_ok(batch, num_entities)) return RGCN_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < rgcn_softmax_workspace_bytes(batch, num_entities, d, slices)) return RGCN_ERR_WORKSPACE;
  RGCN_ALIGN_TRY(16, q, emb, workspace);
  RGCN_ALIGN_TRY(8, target);
  RGCN_ALIGN_TRY(4, allow, query_class, exclude, lse, true_score, row_max, loss, hit);
  hipStream_t stream = (hipStream_t)stream_;
  int* flag = rgcn_index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  const entity_slices p = plan_entity_slices(batch, num_entities, slices, kMaxSlices);
  static bool raised[64] = {};
  const int rc = raise_lds(k_softmax_fwd, (int)kFwdLds, raised);
  if (rc) return rc;
  float* ws_m = (float*)workspace;
  float* ws_l = ws_m + (size_t)p.slices * batch;
  dim3 grid((unsigned)ceil_div64(batch, BM), (unsigned)p.slices);
  k_softmax_fwd<<<grid, kThreads, kFwdLds, stream>>>(q, emb, target, allow, query_class, allow ? (int)num_classes : 0,
                                                     exclude, (int)batch, (int)num_entities, (int)d, p.tiles_per_slice,
                                                     p.num_tiles, ws_m, ws_l, true_score, flag);
  RGCN_HIP_TRY(hipGetLastError());
  k_softmax_merge<<<(unsigned)ceil_div64(batch, kThreads), kThreads, 0, stream>>>(ws_m, ws_l, true_score, (int)batch,
                                                                                 p.slices, lse, row_max, loss, hit);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

int rgcn_softmax_grad(const float* g, const float* q, const float* emb, const int64_t* target, const uint32_t* allow,
                      const int32_t* query_class, int64_t num_classes, const uint32_t* exclude, const float* lse,
                      int64_t batch, int64_t num_entities, int64_t d, int64_t slices, float* dq, float* dE,
                      int accumulate, void* workspace, size_t workspace_bytes, void* stream_) {
  const int bad = check_shape(batch, num_entities, d, slices, num_classes, allow, query_class);
  if (bad) return bad;
  hipStream_t stream = (hipStream_t)stream_;
  if (batch == 0) {
    if (dE && !accumulate) RGCN_HIP_TRY(hipMemsetAsync(dE, 0, (size_t)num_entities * d * sizeof(float), stream));
    return RGCN_OK;
  }
  if (!g || !q || !emb || !target || !lse) return RGCN_ERR_ARG;
  if (!candidate_range_ok(batch, num_entities)) return RGCN_ERR_UNSUPPORTED;
  const entity_slices p = plan_entity_slices(batch, num_entities, slices, kMaxSlices);
  const bool slabs = dq && p.slices > 1;
  if (slabs && (!workspace || workspace_bytes < rgcn_softmax_workspace_bytes(batch, num_entities, d, slices)))
    return RGCN_ERR_WORKSPACE;
  RGCN_ALIGN_TRY(16, q, emb, dq, dE, workspace);
  RGCN_ALIGN_TRY(8, target);
  RGCN_ALIGN_TRY(4, g, lse, allow, query_class, exclude);
  int* flag = rgcn_index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  const int classes = allow ? (int)num_classes : 0;
  const int nb = (int)((d / 32 + 1) / 2);
  if (dq) {
    const size_t slab_floats = (size_t)batch * d;
    dim3 grid((unsigned)ceil_div64(batch, BM), (unsigned)p.slices);
    const int rc = launch_bwd<false>(nb, grid, stream, g, q, emb, target, allow, query_class, classes, exclude, lse,
                                     (int)batch, (int)num_entities, (int)d, p.tiles_per_slice, p.num_tiles,
                                     slabs ? (float*)workspace : dq, slab_floats, 0, flag);
    if (rc) return rc;
    if (slabs) {
      k_softmax_slab_sum<<<(unsigned)ceil_div64((int64_t)slab_floats, kThreads * 4), kThreads, 0, stream>>>(
          (const float*)workspace, slab_floats, p.slices, dq);
      RGCN_HIP_TRY(hipGetLastError());
    }
  }
  if (dE) {
    const int q_tiles = (int)ceil_div64(batch, BN);
    dim3 grid((unsigned)ceil_div64(num_entities, BM), 1u);
    const int rc = launch_bwd<true>(nb, grid, stream, g, emb, q, target, allow, query_class, classes, exclude, lse,
                                    (int)batch, (int)num_entities, (int)d, q_tiles, q_tiles, dE, 0, accumulate ? 1 : 0,
                                    flag);
    if (rc) return rc;
  }
  return RGCN_OK;
}

}  // extern "C"
