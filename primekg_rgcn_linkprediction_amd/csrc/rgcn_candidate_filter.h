// The candidate filter of the passes that walk every entity for every query - top-k (rank_topk.hip) and the 1-vs-all
// softmax, forward and dq (softmax_loss.hip) - and the host checks and slice plan they share with the ranking pass
// (rank_count.hip).  A candidate n of query b is eligible when bit n of allow[query_class[b]] is set (a class outside
// [0, num_classes) allows nothing) and bit n of exclude[b] is clear; either mask may be NULL.  The masks are the bit rows
// of rank_filter.hip: W = ceil(N / 32) words per row, entity n = bit (n & 31) of word (n >> 5).
// Everything sits in an anonymous namespace: each translation unit gets its own copies.
#pragma once
#include "rgcn_common.h"
#include "rgcn_mma_f32_dma.h"

namespace {

// One lane's view of the masks inside mma_f32_dma::walk_tiles: lane li of a wave carries mask row `mrow` (lanes 0-31 and
// 32-63 the same 32 rows, for the first and the second 32-column group of the wave).  load() belongs in the walk's `pre`:
// the words of a column tile are fetched at its first k-tile, from addresses that are always valid (row and word clamped),
// and word() is looked at only in `epi` - a load whose value is needed at once would drain the DMA ring behind it, and the
// counted vmcnt wait of walk_tiles counts these two loads where they stand: allow first, then exclude.
// k_rank_count does not use this: it has one column tile, loads the words after its k loop and only in the lane that
// counts (rank_count.hip, measured).  The dE side of the softmax backward reads the masks transposed and keeps its own.
struct lane_filter {
  const uint32_t* allow;                 // the kernel's arguments: wave-uniform, what load() branches on
  const uint32_t* excl;
  const uint32_t* arow_p;                // this lane's rows
  const uint32_t* erow_p;
  int words;
  bool allowed_row;                      // false: this query's class allows nothing
  unsigned aw, ew;

  __device__ __forceinline__ lane_filter()
      : allow(nullptr), excl(nullptr), arow_p(nullptr), erow_p(nullptr), words(1), allowed_row(true), aw(0xffffffffu), ew(0u) {}
  __device__ __forceinline__ lane_filter(const uint32_t* __restrict__ allow_, const int32_t* __restrict__ qcls,
                                         int num_classes, const uint32_t* __restrict__ excl_, int mrow, int rows, int words_)
      : allow(allow_), excl(excl_), arow_p(allow_), erow_p(nullptr), words(words_), allowed_row(true), aw(0xffffffffu), ew(0u) {
    if (allow) {
      const int c = qcls[min(mrow, rows - 1)];
      allowed_row = c >= 0 && c < num_classes;
      arow_p = allow + (size_t)(allowed_row ? c : 0) * words;
    }
    erow_p = excl ? excl + (size_t)min(mrow, rows - 1) * words : nullptr;
  }
  // the word of the 32-column group that starts at entity first_col (a multiple of 32)
  __device__ __forceinline__ void load(int first_col) {
    const int w = min(first_col >> 5, words - 1);
    if (allow) aw = arow_p[w];
    if (excl) ew = erow_p[w];
  }
  // (a 32-column group wholly past N has no word of its own: its lanes fail the n < N test)
  __device__ __forceinline__ unsigned word() const { return (allowed_row ? aw : 0u) & ~ew; }
};

// ---- host side ----

struct entity_slices {
  int num_tiles, tiles_per_slice, slices;
};

// Slices of the entity range for a grid (row tiles of 64 queries, slices): enough workgroups to fill the machine when
// the batch is small (one row tile: up to one slice per 128-column tile), one slice when the row tiles alone fill it.
// From batch and num_entities alone; `slices` > 0 is the caller's wish, `cap` what the merge behind the pass can take.
inline entity_slices plan_entity_slices(int64_t batch, int64_t num_entities, int64_t slices, int64_t cap) {
  entity_slices p;
  p.num_tiles = (int)ceil_div64(num_entities, mma_f32_dma::KTile<2, mma_f32_dma::B_BLK>::BN);
  const int64_t row_tiles = ceil_div64(batch, mma_f32_dma::BM);
  const int64_t want = slices > 0 ? slices : (row_tiles >= kCUs / 2 ? 1 : ceil_div64(kCUs, row_tiles));
  const rgcn_slicing cut = rgcn_slice_tiles(p.num_tiles, want, cap);
  p.tiles_per_slice = cut.tiles_per_slice;
  p.slices = cut.slices;
  return p;
}

// allow comes with query_class and at least one class (else RGCN_ERR_ARG)
inline bool filter_args_ok(const uint32_t* allow, const int32_t* query_class, int64_t num_classes) {
  return !(num_classes < 0 || (allow && (num_classes == 0 || !query_class)));
}

// rows and columns are 32-bit in the kernels, with room for a tile past the end (else RGCN_ERR_UNSUPPORTED)
inline bool candidate_range_ok(int64_t batch, int64_t num_entities) {
  return !(batch > INT32_MAX / 2 || num_entities > INT32_MAX / 2);
}

}  // namespace
