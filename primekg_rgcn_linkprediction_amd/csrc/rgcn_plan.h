// The chunked work plan the aggregate kernels walk, as plain host code: rowptr -> levels of work items.  No HIP
// include, so that the stand-alone host check (tests/plan_check.cpp, run under AddressSanitizer /
// UndefinedBehaviorSanitizer) plans and executes exactly what rgcn_graph.hip uploads.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/rgcn_hip.h"

// Longest run of source rows one lane group sums sequentially.  At ~1 us per dependent
// round trip and 8 rows in flight per group this bounds a work item to a few us, which is
// what keeps a 25-50 us gather launch free of a straggler tail under Zipf-like degree skew.
constexpr int RGCN_CHUNK = 64;
// Fan-in of the levels above: partial rows are contiguous and a whole workgroup sums one run.
constexpr int RGCN_CHUNK_UP = 512;
constexpr int RGCN_MAX_LEVELS = 8;

// One unit of aggregate work: sum source rows [begin, end) into row `dst`.
//   level 0 : source rows are x[col[e]] for e in [begin, end)
//   level>0 : source rows are partial[begin .. end) (contiguous)
//   flags & RGCN_ITEM_FINAL : `dst` is a final segment row of agg (apply the mean divide), otherwise
//             a row of the partial-sum workspace.
// Level 0 only - packs: a segment longer than RGCN_CHUNK edges is cut into runs of RGCN_CHUNK, and
// up to RGCN_PACK consecutive runs form a pack that sits in RGCN_PACK consecutive, RGCN_PACK-aligned
// item slots - hence inside one gather workgroup for every row width - whose lane groups combine
// their sums through LDS: the pack's first item (the leader) adds the `followers` after it in slot
// order and writes ONE row (final if the whole segment is this pack, a partial row otherwise).
//   RGCN_ITEM_PACK   : slot belongs to a pack (leader, member or padding)
//   RGCN_ITEM_MEMBER : not the leader: contributes through LDS, writes nothing
//   RGCN_ITEM_SKIP   : padding slot of a short pack: nothing to do
//   bits 8..9        : leader only - number of members that follow (0..RGCN_PACK-1)
struct rgcn_item {
  int32_t begin, end, dst, flags;
};
constexpr int RGCN_PACK = 4;
enum : int32_t { RGCN_ITEM_FINAL = 1, RGCN_ITEM_PACK = 2, RGCN_ITEM_MEMBER = 4, RGCN_ITEM_SKIP = 8 };
constexpr int RGCN_ITEM_FOLLOW_SHIFT = 8;

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// What the planner returns: the items of every level, the tile index of a single reduce level (empty otherwise,
// see rgcn_csr::fin_ptr) and the rows of partial-sum workspace all levels use together.
struct rgcn_plan {
  std::vector<std::vector<rgcn_item>> levels;
  std::vector<int32_t> fin_ptr;
  int64_t num_partials = 0;
};

// Host-side plan.  Level 0: a segment of <= RGCN_CHUNK edges is one item; a longer one is cut into
// runs of RGCN_CHUNK edges grouped into packs of RGCN_PACK runs (see above): a pack is summed
// inside one gather workgroup and leaves ONE row - the segment's final row if it is the only pack
// (<= 256 edges), a partial row otherwise.  Levels >= 1 reduce the partial rows of a segment in runs
// of <= RGCN_CHUNK_UP (a workgroup per run) until one row is left.  Order inside level 0: packs first
// (by descending edge count), then the single items by descending length, so the lane groups of a
// wavefront finish together and long items start first; packs occupy RGCN_PACK-aligned slots.
// A third level appears past RGCN_CHUNK * RGCN_PACK * RGCN_CHUNK_UP = 131,072 edges in one segment, a fourth past
// 67,108,864; the int32 edge limit admits no fifth.  Every cut `begin + k * span` is formed in int64 and narrowed
// after the min with the segment's end: in int32 the cut past the end of a segment that ends within a span of 2^31
// overflows.  n_key: nodes that own segments (NR = n_key * R), for fin_ptr's tiles of 32 nodes.
inline int rgcn_build_plan(const std::vector<int32_t>& rowptr, int64_t NR, int64_t R, int64_t n_key, rgcn_plan* plan) {
  struct Pending { int32_t seg, begin, end; };
  struct Pack { int32_t begin, end, dst, final_row; };
  std::vector<std::vector<rgcn_item>>& levels = plan->levels;
  std::vector<Pending> pending, next;
  std::vector<rgcn_item> singles;
  std::vector<Pack> packs;
  int64_t partial_rows = 0;
  levels.clear();
  plan->fin_ptr.clear();
  plan->num_partials = 0;

  for (int64_t s = 0; s < NR; ++s) {
    const int32_t begin = rowptr[s], end = rowptr[s + 1], len = end - begin;
    if (len <= RGCN_CHUNK) {
      singles.push_back({begin, end, (int32_t)s, RGCN_ITEM_FINAL});
      continue;
    }
    const int32_t span = RGCN_CHUNK * RGCN_PACK;
    const int32_t npacks = (int32_t)ceil_div64(len, span);
    if (npacks == 1) {
      packs.push_back({begin, end, (int32_t)s, 1});
    } else {
      const int32_t pbase = (int32_t)partial_rows;
      for (int32_t p = 0; p < npacks; ++p)
        packs.push_back({(int32_t)(begin + (int64_t)p * span),
                         (int32_t)std::min<int64_t>(begin + ((int64_t)p + 1) * span, end), pbase + p, 0});
      partial_rows += npacks;
      pending.push_back({(int32_t)s, pbase, pbase + npacks});
    }
  }
  std::stable_sort(packs.begin(), packs.end(),
                   [](const Pack& a, const Pack& b) { return (a.end - a.begin) > (b.end - b.begin); });
  {  // singles by descending length, stable: lengths are 0..RGCN_CHUNK, so a counting sort does it
    std::vector<int64_t> start(RGCN_CHUNK + 2, 0);
    for (const rgcn_item& it : singles) ++start[RGCN_CHUNK - (it.end - it.begin) + 1];
    for (int l = 0; l <= RGCN_CHUNK; ++l) start[l + 1] += start[l];
    std::vector<rgcn_item> sorted(singles.size());
    for (const rgcn_item& it : singles) sorted[(size_t)start[RGCN_CHUNK - (it.end - it.begin)]++] = it;
    singles.swap(sorted);
  }
  levels.emplace_back();
  levels[0].reserve(packs.size() * RGCN_PACK + singles.size());
  for (const Pack& pk : packs) {
    const int32_t runs = (int32_t)ceil_div64(pk.end - pk.begin, RGCN_CHUNK);
    for (int32_t c = 0; c < RGCN_PACK; ++c) {
      if (c >= runs) {
        levels[0].push_back({0, 0, 0, RGCN_ITEM_PACK | RGCN_ITEM_SKIP});
        continue;
      }
      const int32_t b = pk.begin + c * RGCN_CHUNK, e = (int32_t)std::min<int64_t>((int64_t)b + RGCN_CHUNK, pk.end);
      int32_t flags = RGCN_ITEM_PACK;
      if (c == 0) flags |= (pk.final_row ? RGCN_ITEM_FINAL : 0) | ((runs - 1) << RGCN_ITEM_FOLLOW_SHIFT);
      else flags |= RGCN_ITEM_MEMBER;
      levels[0].push_back({b, e, pk.dst, flags});
    }
  }
  levels[0].insert(levels[0].end(), singles.begin(), singles.end());

  auto emit_up = [&](std::vector<rgcn_item>& out, std::vector<Pending>& nxt, const Pending& p) {
    const int32_t len = p.end - p.begin;
    if (len <= RGCN_CHUNK_UP) {
      out.push_back({p.begin, p.end, p.seg, RGCN_ITEM_FINAL});
      return;
    }
    const int32_t nch = (int32_t)ceil_div64(len, RGCN_CHUNK_UP);
    const int32_t pbase = (int32_t)partial_rows;
    for (int32_t c = 0; c < nch; ++c) {
      const int32_t b = p.begin + c * RGCN_CHUNK_UP;
      out.push_back({b, (int32_t)std::min<int64_t>((int64_t)b + RGCN_CHUNK_UP, p.end), pbase + c, 0});
    }
    partial_rows += nch;
    nxt.push_back({p.seg, pbase, pbase + nch});
  };
  while (!pending.empty()) {
    if ((int)levels.size() >= RGCN_MAX_LEVELS) return RGCN_ERR_UNSUPPORTED;
    levels.emplace_back();
    next.clear();
    for (const Pending& p : pending) emit_up(levels.back(), next, p);
    std::stable_sort(levels.back().begin(), levels.back().end(), [](const rgcn_item& a, const rgcn_item& b) {
      return (a.end - a.begin) > (b.end - b.begin);
    });
    pending.swap(next);
  }
  if (partial_rows > INT32_MAX) return RGCN_ERR_UNSUPPORTED;

  // exactly one reduce level: its items by destination tile, so that a tile-wise consumer can finish them itself
  std::vector<int32_t>& fin_ptr = plan->fin_ptr;
  if (levels.size() == 2 && !levels[1].empty() && R > 0) {
    const int64_t tiles = ceil_div64(n_key, 32);
    auto tile_of = [&](const rgcn_item& it) { return (int64_t)(it.dst / R) >> 5; };
    std::stable_sort(levels[1].begin(), levels[1].end(),
                     [&](const rgcn_item& a, const rgcn_item& b) { return tile_of(a) < tile_of(b); });
    fin_ptr.assign((size_t)tiles + 1, 0);
    for (const rgcn_item& it : levels[1]) ++fin_ptr[(size_t)tile_of(it) + 1];
    for (int64_t t = 0; t < tiles; ++t) fin_ptr[(size_t)t + 1] += fin_ptr[(size_t)t];
  }
  plan->num_partials = partial_rows;
  return RGCN_OK;
}
