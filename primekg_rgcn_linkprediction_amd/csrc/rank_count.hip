// Link ranking without the [B, N] score matrix (evaluate.py:260-276 of the reference, and its filtered,
// type-constrained form): row m is a query, column n a candidate entity; count the candidates that beat the true
// entity's score.
//
//   score[m, n] = <q[m], emb[n]>  - the shared fp32 LDS-DMA k-tile (rgcn_mma_f32_dma.h) with one A operand and one
//                                   B_BLK block, so a score here, the one distmult_score_all_tails stores
//                                   (k_gemm_nt_dma<2, B_BLK>) and the one k_topk_select keeps are the same bits
//   counted     = n < N, n != target[m], NOT (score <= true_score[m]), allowed (allow[query_class[m]]), not excluded
//                 (exclude[m]); the masks are bit rows, bit (n & 31) of word (n >> 5) - see rank_filter.hip
//   non-finite  = without NaN "not <=" is ">", infinities included (equal scores do not count: +inf against +inf,
//                 -inf against -inf), so finite data counts as it always did.  A NaN candidate counts against every
//                 true score (where torch's descending argsort puts it); a NaN true score is beaten by every eligible
//                 candidate: rank = 1 + #eligible, never a good rank for a missing value (include/rgcn_hip.h)
//
// A workgroup has ONE column tile, so the k loop below is the one-column-tile case of mma_f32_dma::walk_tiles
// (rgcn_mma_f32_dma.h) written out: same wait, barrier, read_first, stage t + 2, finish - and a change to the wait
// discipline there has to be made here too.  On the walk itself the kernel was measured 28 % slower (the raw launch
// at B = 15,372, N = 30,926, d = 128: 1.645 -> 2.109 ms, profiles/tile_walk_shared.txt): there the epilogue sits
// inside the loop, and the kernel came out at 186 VGPRs and 2,669 instructions against 150 and 2,399 here.
#include "rgcn_candidate_filter.h"    // and with it rgcn_common.h and rgcn_mma_f32_dma.h

namespace {

using namespace mma_f32_dma;

constexpr int kRankTN = 2;              // 64 x 128 scores per workgroup

// grid (ceil(M / 64), ceil(N / 128)); beaten_by is zeroed by the caller and receives one atomicAdd per (row,
// 32-column group) with a hit.  allow ([num_classes, ceil(N / 32)] words, with query_class) and exclude
// ([M, ceil(N / 32)] words) may each be NULL; d is a multiple of 32.
__global__ __launch_bounds__(kThreads) void k_rank_count(const float* __restrict__ q, const float* __restrict__ emb,
                                                         const float* __restrict__ true_score,
                                                         const int64_t* __restrict__ target,
                                                         const uint32_t* __restrict__ allow,
                                                         const int32_t* __restrict__ query_class, int num_classes,
                                                         const uint32_t* __restrict__ exclude,
                                                         int32_t* __restrict__ beaten_by, int M, int N, int d) {
  constexpr int TN = kRankTN;
  typedef KTile<TN, B_BLK> Tile;
  constexpr int BN = Tile::BN, A_FLOATS = Tile::A_FLOATS, BUF_FLOATS = Tile::BUF_FLOATS;
  constexpr int A_PW = Tile::A_PW, B_PW = Tile::B_PW, P = Tile::P;
  __shared__ __attribute__((aligned(16))) float lds[NBUF * BUF_FLOATS];   // the ONLY LDS object

  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;

  floatx16 acc[TN];
#pragma unroll
  for (int b = 0; b < TN; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

  // per-lane source offsets, fixed over the k loop
  size_t a_off[A_PW], b_off[B_PW];
#pragma unroll
  for (int j = 0; j < A_PW; ++j) {
    const int row = dma_row(wave * A_PW + j, lane);
    a_off[j] = (size_t)min(m0 + row, M - 1) * d + dma_col(row, lane);   // rows past M read a valid row; never counted
  }
#pragma unroll
  for (int j = 0; j < B_PW; ++j) {
    const int row = dma_row(wave * B_PW + j, lane);
    b_off[j] = (size_t)min(n0 + row, N - 1) * d + dma_col(row, lane);   // columns past N likewise
  }
  auto stage = [&](int kt, int buf) {
    float* sA = lds + buf * BUF_FLOATS;
    float* sB = sA + A_FLOATS;
#pragma unroll
    for (int j = 0; j < A_PW; ++j) glds16(q + kt + a_off[j], sA + (wave * A_PW + j) * 8 * BK);
#pragma unroll
    for (int j = 0; j < B_PW; ++j) glds16(emb + kt + b_off[j], sB + (wave * B_PW + j) * 8 * BK);
  };

  stage(0, 0);
  if (BK < d) stage(BK, 1);

  Tile tile(wm, wn, li, lh);

  int t = 0;
  for (int kt = 0; kt < d; kt += BK, ++t) {
    // k-tile kt landed for this wave (all but the newest P DMAs are done), then for all waves;
    // the barrier also says every wave is done reading the buffer the next stage() overwrites
    if (kt + BK < d) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const unsigned buf_bytes = Tile::buf_bytes(t % NBUF);
    tile.read_first(buf_bytes);
    if (kt + 2 * BK < d) stage(kt + 2 * BK, (t + 2) % NBUF);
    tile.finish(acc, buf_bytes);
  }

  // The ballot of an accumulator register is the 32 hits of columns nb .. nb+31 of two rows (lanes 0-31 / 32-63),
  // and nb is a multiple of 32: exactly one word of a [rows, ceil(N/32)] bit mask per row, so the filter is
  // hits & allow[class[m]][w] & ~exclude[m][w] before the popcount - two 4-byte loads per (row, 32-column group), all
  // issued before the group's ballots.  A target outside [0, N) excludes nothing.
  const int words = (N + 31) >> 5;
  constexpr unsigned kNoRow = 0xffffffffu;
  float ts[16];
  int tl[16];
  unsigned aoff[16];                     // first word of the row's allow row, kNoRow: nothing is allowed
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + acc_row(r, lh);
    const bool ok = m < M;
    ts[r] = ok ? true_score[m] : 0.f;
    const int64_t t64 = ok ? target[m] : -1;
    tl[r] = (t64 >= 0 && t64 < N) ? (int)t64 : -1;
    aoff[r] = kNoRow;
    if (allow && ok) {
      const int c = query_class[m];
      if (c >= 0 && c < num_classes) aoff[r] = (unsigned)c * (unsigned)words;
    }
  }
#pragma unroll
  for (int b = 0; b < TN; ++b) {
    const int nb = n0 + (wn * TN + b) * 32, n = nb + li;
    const int w = nb >> 5;
    const bool wok = w < words;          // a column group wholly past N has no mask word (and no hit)
    unsigned aw[16], ew[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 32 + acc_row(r, lh);
      // only the lane that counts (li == 0 of each half) needs the words
      aw[r] = allow ? ((li == 0 && wok && aoff[r] != kNoRow) ? allow[aoff[r] + (unsigned)w] : 0u) : 0xffffffffu;
      ew[r] = (li == 0 && exclude && wok && m < M) ? exclude[(size_t)m * words + w] : 0u;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 32 + acc_row(r, lh);
      // counted UNLESS score <= true score: a NaN on either side counts (the > form would count neither)
      const unsigned long long hits = __ballot(m < M && n < N && n != tl[r] && !(acc[b][r] <= ts[r]));
      if (li == 0 && m < M) {
        const unsigned mine = lh ? (unsigned)(hits >> 32) : (unsigned)hits;
        const int c = __popc(mine & aw[r] & ~ew[r]);
        if (c) atomicAdd(&beaten_by[m], c);
      }
    }
  }
}

// the one launch behind both entry points; each keeps its own argument checks
int launch_rank_count(const float* q, const float* emb, const float* true_score, const int64_t* target,
                      const uint32_t* allow, const int32_t* query_class, int64_t num_classes, const uint32_t* exclude,
                      int64_t batch, int64_t num_entities, int64_t d, int32_t* beaten_by, void* stream) {
  RGCN_ALIGN_TRY(16, q, emb);                    // the k-tiles arrive in 16-byte DMA pieces; the epilogue reads words
  RGCN_ALIGN_TRY(8, target);
  RGCN_ALIGN_TRY(4, true_score, allow, query_class, exclude, beaten_by);
  dim3 grid((unsigned)ceil_div64(batch, BM), (unsigned)ceil_div64(num_entities, KTile<kRankTN, B_BLK>::BN));
  k_rank_count<<<grid, kThreads, 0, (hipStream_t)stream>>>(q, emb, true_score, target, allow, query_class,
                                                           allow ? (int)num_classes : 0, exclude, beaten_by, (int)batch,
                                                           (int)num_entities, (int)d);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace

extern "C" {

int distmult_rank_tails(const float* hr, const float* emb, const float* true_score, const int64_t* tail,
                        int64_t batch, int64_t num_entities, int64_t d, int32_t* beaten_by, void* stream_) {
  if (batch < 0 || num_entities <= 0 || d <= 0 || (d % BK)) return (d > 0 && (d % BK)) ? RGCN_ERR_UNSUPPORTED : RGCN_ERR_ARG;
  if (batch == 0) return RGCN_OK;
  if (!hr || !emb || !true_score || !tail || !beaten_by) return RGCN_ERR_ARG;
  if (!candidate_range_ok(batch, num_entities)) return RGCN_ERR_UNSUPPORTED;
  return launch_rank_count(hr, emb, true_score, tail, nullptr, nullptr, 0, nullptr, batch, num_entities, d, beaten_by,
                           stream_);
}

int distmult_rank_masked(const float* q, const float* emb, const float* true_score, const int64_t* target,
                         const uint32_t* allow, const int32_t* query_class, int64_t num_classes, const uint32_t* exclude,
                         int64_t batch, int64_t num_entities, int64_t d, int32_t* beaten_by, void* stream_) {
  if (batch < 0 || num_entities <= 0 || d <= 0 || (d % BK)) return (d > 0 && (d % BK)) ? RGCN_ERR_UNSUPPORTED : RGCN_ERR_ARG;
  if (!filter_args_ok(allow, query_class, num_classes)) return RGCN_ERR_ARG;
  if (batch == 0) return RGCN_OK;
  if (!q || !emb || !true_score || !target || !beaten_by) return RGCN_ERR_ARG;
  if (!candidate_range_ok(batch, num_entities)) return RGCN_ERR_UNSUPPORTED;
  const int64_t words = ceil_div64(num_entities, 32);
  if (allow && num_classes * words > INT32_MAX) return RGCN_ERR_UNSUPPORTED;   // 32-bit word offsets in the epilogue
  return launch_rank_count(q, emb, true_score, target, allow, query_class, num_classes, exclude, batch, num_entities, d,
                           beaten_by, stream_);
}

}  // extern "C"
