// Top-k candidates per query from the ranking pass's scores, without the [B, N] score matrix
// (case_studies.predict_top_drugs / medical_validation.generate_predictions + _filter_known_associations of the
// reference: "which entities, allowed and not already linked, does the model score highest for this query?").
//
//   score[b, n] = <q[b], emb[n]>   - the k-tile of k_gemm_nt_dma<2, B_BLK> (rgcn_transform.hip), shared
//                                    (rgcn_mma_f32_dma.h): the same LDS-DMA ring, fragment reads and
//                                    v_mfma_f32_32x32x2_f32 sequence per output element, so a score here and the one
//                                    distmult_score_all_tails stores are the same bits
//   candidates  = allowed (allow[query_class[b]]), not excluded (exclude[b]), not NaN, >= min_score
//   order       = score descending, equal scores by entity id ascending
//
// Select pass, grid (ceil(B / 64), S): a workgroup owns 64 query rows and walks the 128-column tiles of slice s of
// the entity range, ids ascending.  The (column tile, k-tile) pairs form ONE stream through the three-buffer ring,
// so the DMA pipeline never drains between column tiles: the walk is mma_f32_dma::walk_tiles (rgcn_mma_f32_dma.h), the
// mask-word loads its `pre`, the selection its `epi`.  After the last k-tile of a column tile the accumulators
// are tested against the row's current k-th best score (one ballot per accumulator register, filtered by one mask
// word per row and 32-column group exactly as k_rank_count does) and the survivors - about k ln(N / k) per row
// over the whole walk - are inserted by the whole wave into the row's sorted list in LDS.
//   One list per ROW: the two waves that share a row (wave columns 0 and 1) insert one after the other - wave
//   column 0, a barrier, wave column 1 - so every row sees ONE stream of candidates with ascending ids, and
//   "insert only if strictly greater than the k-th best, after the entries that are >=" is the tie rule.
// Merge pass, one workgroup per row: a k-round S-way merge of the row's slice lists by the total order.
#include <math.h>

#include "rgcn_candidate_filter.h"    // and with it rgcn_common.h and rgcn_mma_f32_dma.h

namespace {

using namespace mma_f32_dma;    // kThreads (256: 4 waves, 2 (m) x 2 (n)), BK, BM, NBUF, walk_tiles, acc_row, the vector types

typedef KTile<2, B_BLK> Tile;   // 64 x 128 outputs per workgroup, B = embedding rows
constexpr int BN = Tile::BN, BUF_FLOATS = Tile::BUF_FLOATS;
constexpr int STAGE_BYTES = NBUF * BUF_FLOATS * 4;               // 73,728
constexpr int kMaxK = 128;      // list length the select pass is built for (two entries per lane of the inserting wave)
constexpr int kMaxSlices = 256; // one list per thread of the merge workgroup

// dynamic LDS of the select pass: [ring 73,728 B][thr f32 x 64][cnt i32 x 64][scores f32 x 64 k][ids i32 x 64 k]
__host__ __device__ inline size_t select_lds_bytes(int k) { return (size_t)STAGE_BYTES + 2 * BM * 4 + (size_t)BM * k * 8; }

// Insert (s, id) into the sorted list of `row`, by all 64 lanes of a wave.  thr[row] is the k-th best score once
// the list is full and NaN before (NaN rejects nothing); s is never NaN.  Entries with a score >= s stay in front:
// an equal score that came earlier (a smaller id) keeps its place.
// The lanes talk to each other through LDS here (one lane's store is another lane's next load), which the language
// does not promise without a fence: every access is volatile, so none is hoisted, forwarded or dropped, and an LDS
// operation of a wave completes in program order.
typedef volatile __attribute__((address_space(3))) float* lds_vfloat;     // the address space spelled out: a volatile
typedef volatile __attribute__((address_space(3))) int* lds_vint;         // generic pointer would become flat accesses
__device__ inline void list_insert(lds_vfloat s_thr, lds_vint s_cnt, lds_vfloat l_score, lds_vint l_id, int row, int k,
                                   float s, int id, int lane) {
  // two LDS round trips per insertion: (threshold, length), then the list; the stores need no wait - the next
  // insertion's loads queue behind them
  const float thr = s_thr[row];
  const int cnt = s_cnt[row];
  if (s <= thr) return;                               // wave-uniform
  lds_vfloat rs = l_score + row * k;
  lds_vint ri = l_id + row * k;
  const int i0 = lane, i1 = lane + 64;
  const bool h0 = i0 < cnt, h1 = i1 < cnt;
  float s0 = 0.f, s1 = 0.f;
  int d0 = 0, d1 = 0;
  if (h0) { s0 = rs[i0]; d0 = ri[i0]; }
  if (h1) { s1 = rs[i1]; d1 = ri[i1]; }
  const int p = __popcll(__ballot(h0 && s0 >= s)) + __popcll(__ballot(h1 && s1 >= s));   // < k: the list is not full or s > its last
  if (h0 && i0 >= p && i0 + 1 < k) { rs[i0 + 1] = s0; ri[i0 + 1] = d0; }
  if (h1 && i1 >= p && i1 + 1 < k) { rs[i1 + 1] = s1; ri[i1 + 1] = d1; }
  // the list's new last entry, once it is full: s itself, or what stood at k - 2 and has just moved down
  float last = s;
  if (cnt + 1 >= k && p < k - 1) {
    const int src = k - 2;                            // >= 0 here (p >= 0 < k - 1), < cnt
    last = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(src < 64 ? s0 : s1), src & 63));
  }
  if (lane == 0) {
    rs[p] = s;
    ri[p] = id;
    if (cnt < k) s_cnt[row] = cnt + 1;
    if (cnt + 1 >= k) s_thr[row] = last;
  }
}

__global__ __launch_bounds__(kThreads) void k_topk_select(const float* __restrict__ q, const float* __restrict__ emb,
                                                          const uint32_t* __restrict__ allow,
                                                          const int32_t* __restrict__ qcls, int num_classes,
                                                          const uint32_t* __restrict__ excl, float min_score, int M,
                                                          int N, int d, int k, int tiles_per_slice, int num_tiles,
                                                          float* __restrict__ ws_score, int* __restrict__ ws_id) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* s_thr = lds + NBUF * BUF_FLOATS;
  int* s_cnt = reinterpret_cast<int*>(s_thr + BM);
  float* l_score = s_thr + 2 * BM;
  int* l_id = reinterpret_cast<int*>(l_score + BM * k);

  const int m0 = blockIdx.x * BM;
  const int ct_begin = blockIdx.y * tiles_per_slice, ct_end = min(num_tiles, ct_begin + tiles_per_slice);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int words = (N + 31) >> 5;

  if (tid < BM) {
    s_thr[tid] = __builtin_nanf("");
    s_cnt[tid] = 0;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // landed before the first barrier of the walk, which every epilogue follows

  // this lane's mask row: lanes 0-31 carry the first 32-column group of the wave, lanes 32-63 the second
  lane_filter filt(allow, qcls, num_classes, excl, m0 + wm * 32 + li, M, words);

  Tile tile(wm, wn, li, lh);

  // Selection epilogue of column tile ct (the accumulators hold its 64 x 128 scores).  Fast part, straight-line:
  // every lane tests its 32 scores against the rows' thresholds and keeps the outcomes as 32 bits.  Once the lists
  // are full almost every wave leaves here.  Otherwise the slow part walks the accumulator registers that have a hit
  // in a rolled loop (one copy of the insertion code): ballot, mask words, one insertion per surviving bit.
  auto select = [&](int ct, floatx16 (&acc)[2], unsigned okw) {
    float thr[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(&s_thr[wm * 32 + acc_row(4 * g, lh)]);   // registers 4 g .. 4 g + 3
      thr[4 * g + 0] = v.x; thr[4 * g + 1] = v.y; thr[4 * g + 2] = v.z; thr[4 * g + 3] = v.w;
    }
    unsigned mybits = 0;                                       // bit b * 16 + r: acc[b][r] of this lane is a hit
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const bool nok = ct * BN + (wn * 2 + b) * 32 + li < N;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + acc_row(r, lh);
        const float v = acc[b][r];
        const bool hit = nok & (m < M) & (v >= min_score) & !(v <= thr[r]);   // no short circuit: straight-line code
        mybits |= (unsigned)hit << (b * 16 + r);
      }
    }
    if (__ballot(mybits != 0) == 0) return;
    unsigned anybits = mybits;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) anybits |= __shfl_xor(anybits, o);
    anybits = __builtin_amdgcn_readfirstlane(anybits);
    while (anybits) {                                          // wave-uniform; registers in (b, r) order: ids ascend per row
      const int pb = __builtin_ctz(anybits);
      anybits &= anybits - 1;
      const int b = pb >> 4, r = pb & 15;
      const int nb = ct * BN + (wn * 2 + b) * 32;
      float v = 0.f;
      switch (pb) {
#define TOPK_CASE(B_, R_) case (B_) * 16 + (R_): v = acc[B_][R_]; break;
#define TOPK_CASES(B_) TOPK_CASE(B_, 0) TOPK_CASE(B_, 1) TOPK_CASE(B_, 2) TOPK_CASE(B_, 3) TOPK_CASE(B_, 4) TOPK_CASE(B_, 5) \
  TOPK_CASE(B_, 6) TOPK_CASE(B_, 7) TOPK_CASE(B_, 8) TOPK_CASE(B_, 9) TOPK_CASE(B_, 10) TOPK_CASE(B_, 11)                 \
  TOPK_CASE(B_, 12) TOPK_CASE(B_, 13) TOPK_CASE(B_, 14) TOPK_CASE(B_, 15)
        TOPK_CASES(0) TOPK_CASES(1)
#undef TOPK_CASES
#undef TOPK_CASE
      }
      const unsigned long long hits = __ballot((mybits >> pb) & 1u);
      for (int h = 0; h < 2; ++h) {
        const int rowl = acc_row(r, h);                        // the row of this half inside the wave's 32
        const unsigned word = (unsigned)__builtin_amdgcn_readlane((int)okw, b * 32 + rowl);
        unsigned mine = (h ? (unsigned)(hits >> 32) : (unsigned)hits) & word;
        while (mine) {                                         // bits (= ids) ascending
          const int bit = __builtin_ctz(mine);
          mine &= mine - 1;
          const float s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), h * 32 + bit));
          list_insert((lds_vfloat)s_thr, (lds_vint)s_cnt, (lds_vfloat)l_score, (lds_vint)l_id, wm * 32 + rowl, k, s,
                      nb + bit, lane);
        }
      }
    }
  };

  // the column tile's mask words, one (row, 32-column group) per lane, a column tile ahead of their use
  auto pre = [&](int ct) { filt.load(ct * BN + (wn * 2 + lh) * 32); };
  auto epi = [&](int ct, floatx16 (&acc)[2]) {
    // wave column 0 selects, then wave column 1: one stream of ascending ids per row.  Every wave passes exactly
    // one barrier here; the list writes of the first are complete (lgkmcnt(0)) before it, and those of the second
    // before the barrier that opens the next k-tile.
    if (wn == 1) {
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    select(ct, acc, filt.word());
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (wn == 0) __builtin_amdgcn_s_barrier();
  };
  // rows past M and columns past N read a valid row; never selected
  walk_tiles(lds, q, emb, M, d, m0, ct_begin, ct_end, wave, lane, tile, [&](int n) { return min(n, N - 1); }, pre, epi);
  __syncthreads();

  // the lists of this slice -> workspace [B][S][k]; slots past a list's length carry id -1
  const int S = gridDim.y;
  for (int e = tid; e < BM * k; e += kThreads) {
    const int row = e / k, j = e - row * k, m = m0 + row;
    if (m >= M) break;
    const bool has = j < s_cnt[row];
    const size_t o = ((size_t)m * S + blockIdx.y) * k + j;
    ws_score[o] = has ? l_score[e] : -INFINITY;
    ws_id[o] = has ? l_id[e] : -1;
  }
}

// 64-bit key whose descending order is (score descending, id ascending); > 0 for every real entry
__device__ inline unsigned long long order_key(float s, int id) {
  unsigned u = __float_as_uint(s + 0.f);                       // -0.0 -> +0.0: the two compare equal
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return ((unsigned long long)u << 32) | (unsigned)(~id);
}

// One workgroup per query row: thread t walks the list of slice t (sorted by the total order); k rounds of
// "the best head wins, its owner advances".  S == 1: the list is the answer.
__global__ __launch_bounds__(kThreads) void k_topk_merge(const float* __restrict__ ws_score, const int* __restrict__ ws_id,
                                                         int S, int k, int64_t* __restrict__ top_ids,
                                                         float* __restrict__ top_scores) {
  __shared__ unsigned long long s_best[2][kThreads / 64];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t* oid = top_ids + (size_t)row * k;
  float* osc = top_scores + (size_t)row * k;
  if (S == 1) {
    for (int j = tid; j < k; j += kThreads) {
      const int id = ws_id[(size_t)row * k + j];
      oid[j] = id;                                             // -1 past the list's length
      osc[j] = id >= 0 ? ws_score[(size_t)row * k + j] : -INFINITY;
    }
    return;
  }
  const size_t base = ((size_t)row * S + tid) * k;
  int pos = 0, id = -1;
  float sc = 0.f;
  unsigned long long key = 0;
  auto load_head = [&]() {
    key = 0;
    if (tid < S && pos < k) {
      id = ws_id[base + pos];
      if (id >= 0) {
        sc = ws_score[base + pos];
        key = order_key(sc, id);
      }
    }
  };
  load_head();
  for (int j = 0; j < k; ++j) {
    unsigned long long best = key;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(best, o);
      best = other > best ? other : best;
    }
    if (lane == 0) s_best[j & 1][wave] = best;
    __syncthreads();                                           // (two buffers: round j + 1 writes the other one)
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) best = s_best[j & 1][w] > best ? s_best[j & 1][w] : best;
    if (best == 0) {                                           // every list is used up: padding from here on
      for (int jj = j + tid; jj < k; jj += kThreads) {
        oid[jj] = -1;
        osc[jj] = -INFINITY;
      }
      return;
    }
    if (key == best) {                                         // exactly one thread: ids are distinct
      oid[j] = id;
      osc[j] = sc;
      ++pos;
      load_head();
    }
  }
}

}  // namespace

extern "C" {

size_t distmult_topk_workspace_bytes(int64_t batch, int64_t num_entities, int64_t k, int64_t slices) {
  if (batch <= 0 || num_entities <= 0 || k <= 0 || slices < 0) return 0;
  const entity_slices p = plan_entity_slices(batch, num_entities, slices, kMaxSlices);
  return (size_t)batch * p.slices * k * (sizeof(float) + sizeof(int32_t));
}

int distmult_topk_masked(const float* q, const float* emb, const uint32_t* allow, const int32_t* query_class,
                         int64_t num_classes, const uint32_t* exclude, float min_score, int64_t batch,
                         int64_t num_entities, int64_t d, int64_t k, int64_t slices, int64_t* top_ids, float* top_scores,
                         void* workspace, size_t workspace_bytes, void* stream_) {
  if (batch < 0 || num_entities <= 0 || d <= 0 || (d % BK)) return (d > 0 && (d % BK)) ? RGCN_ERR_UNSUPPORTED : RGCN_ERR_ARG;
  if (k <= 0 || slices < 0 || min_score != min_score) return RGCN_ERR_ARG;
  if (!filter_args_ok(allow, query_class, num_classes)) return RGCN_ERR_ARG;
  if (batch == 0) return RGCN_OK;
  if (!q || !emb || !top_ids || !top_scores) return RGCN_ERR_ARG;
  if (k > kMaxK) return RGCN_ERR_UNSUPPORTED;
  if (!candidate_range_ok(batch, num_entities) || d > (1 << 24)) return RGCN_ERR_UNSUPPORTED;
  const int64_t words = ceil_div64(num_entities, 32);
  if (allow && num_classes * words > INT32_MAX) return RGCN_ERR_UNSUPPORTED;   // 32-bit word offsets in the epilogue
  if (!workspace || workspace_bytes < distmult_topk_workspace_bytes(batch, num_entities, k, slices)) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(16, q, emb, workspace);         // 16-byte DMA pieces of the k-tiles; the lists and masks go word by word
  RGCN_ALIGN_TRY(8, top_ids);
  RGCN_ALIGN_TRY(4, allow, query_class, exclude, top_scores);
  hipStream_t stream = (hipStream_t)stream_;
  const entity_slices p = plan_entity_slices(batch, num_entities, slices, kMaxSlices);
  const size_t lds_bytes = select_lds_bytes((int)k);
  static bool raised[64] = {};
  const int rc = raise_lds(k_topk_select, (int)select_lds_bytes(kMaxK), raised);
  if (rc) return rc;
  float* ws_score = (float*)workspace;
  int* ws_id = (int*)(ws_score + (size_t)batch * p.slices * k);
  dim3 grid((unsigned)ceil_div64(batch, BM), (unsigned)p.slices);
  k_topk_select<<<grid, kThreads, lds_bytes, stream>>>(q, emb, allow, query_class, allow ? (int)num_classes : 0, exclude,
                                                       min_score, (int)batch, (int)num_entities, (int)d, (int)k,
                                                       p.tiles_per_slice, p.num_tiles, ws_score, ws_id);
  RGCN_HIP_TRY(hipGetLastError());
  k_topk_merge<<<(unsigned)batch, kThreads, 0, stream>>>(ws_score, ws_id, p.slices, (int)k, top_ids, top_scores);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // extern "C"
