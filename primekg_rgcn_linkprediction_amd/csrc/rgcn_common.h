// Shared declarations for librgcn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/rgcn_hip.h"
#include "rgcn_plan.h"

#define RGCN_HIP_TRY(expr)                       \
  do {                                           \
    hipError_t err__ = (expr);                   \
    if (err__ != hipSuccess) return RGCN_ERR_HIP; \
  } while (0)

// The alignment contract of the C boundary (include/rgcn_hip.h, "Alignment"): every entry point, once its other
// argument checks have passed and before its first HIP runtime call, refuses a pointer whose address is not a
// multiple of the widest single access a kernel makes through it.  `a`: a power of two; NULL passes (optional
// operands).  A handful of integer ORs and one AND on the host.
template <class... P>
static inline bool rgcn_aligned(uintptr_t a, P... p) {
  uintptr_t bits = 0;
  ((bits |= (uintptr_t)(const void*)p), ...);
  return (bits & (a - 1)) == 0;
}
#define RGCN_ALIGN_TRY(a, ...)                                       \
  do {                                                               \
    if (!rgcn_aligned((a), __VA_ARGS__)) return RGCN_ERR_ALIGN;      \
  } while (0)

// ---------------------------------------------------------------------------------------------
// Host scaffolding of the launches, one copy each.
// ---------------------------------------------------------------------------------------------
constexpr int kCUs = 256;       // MI355X

// workspace sections start on 256-byte boundaries
static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// The slice rule of the kernels that walk a range of column tiles (top-k select, silhouette, t-SNE repulsion): `tiles`
// tiles cut into at most min(want, cap) slices of equal length, the last one shorter, none empty.  `want` is what the
// caller was asked for or, for "choose yourself", its own default - the defaults differ on measured grounds.
struct rgcn_slicing {
  int tiles_per_slice, slices;
};
static inline rgcn_slicing rgcn_slice_tiles(int64_t tiles, int64_t want, int64_t cap) {
  const int64_t most = tiles < cap ? tiles : cap;
  want = want < most ? want : most;
  want = want > 1 ? want : 1;
  const int64_t per = (tiles + want - 1) / want;
  return {(int)per, (int)((tiles + per - 1) / per)};
}

// A launch may ask for 64 KB of dynamic LDS by default and the three-buffer ring of the fp32 k-tile is more: the limit
// of `kernel` is raised to `bytes` once per device (`raised`: the caller's static flags; not a stream operation).
template <class K>
static inline int raise_lds(K kernel, int bytes, bool (&raised)[64]) {
  int dev = 0;
  RGCN_HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !raised[dev]) {
    RGCN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (dev >= 0 && dev < 64) raised[dev] = true;
  }
  return RGCN_OK;
}

// The parameter gradients of a layer over an empty graph (N == 0): all zero, nothing to launch.
static inline int rgcn_zero_param_grads(float* grad_weight, float* grad_root, float* grad_bias, int64_t R, int64_t d_in,
                                        int64_t d_out, hipStream_t stream) {
  RGCN_HIP_TRY(hipMemsetAsync(grad_weight, 0, (size_t)(R * d_in) * d_out * sizeof(float), stream));
  if (grad_root) RGCN_HIP_TRY(hipMemsetAsync(grad_root, 0, (size_t)d_in * d_out * sizeof(float), stream));
  if (grad_bias) RGCN_HIP_TRY(hipMemsetAsync(grad_bias, 0, (size_t)d_out * sizeof(float), stream));
  return RGCN_OK;
}

// The work plan's constants and item record live in rgcn_plan.h (plain host code, shared with the host check).
// Edges of an item whose ids travel with the item (= rows a lane group keeps in flight).
constexpr int RGCN_HEAD = 8;

struct rgcn_csr {
  int32_t* rowptr = nullptr;  // [N*R+1]
  int32_t* col = nullptr;     // [E]  the other endpoint
  int64_t* perm = nullptr;    // [E]  original column of each bucketed edge
  float* val = nullptr;       // cnt[n_key*R] (mean mode) or w[E] (weighted-sum mode)
  bool weighted = false;      // false: agg = sum / cnt (mean); true: agg = sum of w[e] * row
  int64_t n_key = 0;          // nodes that own segments (rows of agg = n_key * R)
  int64_t n_other = 0;        // nodes the col[] ids refer to (rows of x)
  int num_levels = 0;
  // Where the live level-0 slots end, counted from the back: the plan orders level 0 as packs, then singles by
  // descending length, so the segments without an edge are exactly the last empty_items0 items and the slots in front
  // of the first empty single are num_items[0] - empty_items0.  The gather launch walks those and only stores zero
  // rows for the rest (rgcn_aggregate.hip).  At most n_key * R < 2^31; an int32 here leaves every other field where
  // it was (the mirror of this struct in tests/test_alignment_host.py).
  int32_t empty_items0 = 0;
  rgcn_item* items[RGCN_MAX_LEVELS] = {};
  int64_t num_items[RGCN_MAX_LEVELS] = {};
  int64_t num_partials = 0;   // rows of partial-sum workspace (all levels)
  // Per level-0 item, the column ids (and, in weighted mode, the weights) of its first RGCN_HEAD
  // edges, padded with -1 / 0: fetched together with the item record, so the first row loads of an
  // item are one dependent round trip away instead of two (item -> col -> row).
  int32_t* head_col = nullptr;   // [num_items[0] * RGCN_HEAD]
  float* head_w = nullptr;       // [num_items[0] * RGCN_HEAD], weighted structures only
  // bit r of tile_mask[t]: some row of rows [32t, 32t+32) has a non-empty (row, r) segment.
  // Typed relations leave whole row ranges without a relation (drug-gene edges never reach a
  // disease row): the transforms skip the all-zero k/m-tiles these bits expose.  NULL if R > 32.
  // The SAME allocation carries the occupancy row by row behind the tile words (rgcn_row_mask_offset): bit r of
  // row_mask[i] says segment (i, r) has an edge, so tile_mask[t] is the OR of its 32 rows; zero words pad it for
  // the rows a consumer's last tiles reach past n_key.  A consumer of a sparse aggregate (rgcn_hip.h,
  // RGCN_MODE_SPARSE_ROWS) finds it from tile_mask and its own row count - no field of this struct moves.
  uint32_t* tile_mask = nullptr;
  int64_t num_row_tiles = 0;
  // Deferred hub tails: when the plan has exactly ONE reduce level (every segment <= RGCN_CHUNK * RGCN_PACK *
  // RGCN_CHUNK_UP = 131,072 edges), its items are ordered by the 32-row tile of their destination row and
  // fin_ptr[t] .. fin_ptr[t + 1] are the items of tile t: a consumer that reads the aggregate tile by tile (the
  // split-precision NT transforms) can finish the hub rows of its own tile itself - the same sums in the same
  // order as k_reduce_partials - and the separate reduce launch disappears.  NULL otherwise.
  int32_t* fin_ptr = nullptr;   // [num_fin_tiles + 1]
  int64_t num_fin_tiles = 0;
  // max over segments of sum of |weights| (weighted mode; 1 in mean mode): |agg row| <= weight_bound * max |x|.
  // The split-precision transforms scale the aggregate operand by this bound instead of scanning it.
  float weight_bound = 1.f;
};

static_assert(offsetof(rgcn_csr, items) == offsetof(rgcn_csr, num_levels) + 8, "empty_items0 sits behind num_levels");

// Layout of the occupancy allocation of a structure with n_key rows: ceil(n_key / 32) tile words, padded to a
// 16-byte boundary, then n_key row words and RGCN_ROW_MASK_PAD zero words (a consumer stages up to two 32-row tiles
// past its last row and reads four words at a time).
constexpr int64_t RGCN_ROW_MASK_PAD = 96;
static inline int64_t rgcn_row_mask_offset(int64_t n_key) { return ((n_key + 31) / 32 + 3) / 4 * 4; }
static inline int64_t rgcn_occupancy_words(int64_t n_key) { return rgcn_row_mask_offset(n_key) + n_key + RGCN_ROW_MASK_PAD; }
// Host side of both masks, from a host copy of rowptr [n_key * R + 1]: `words` = rgcn_occupancy_words(n_key), zeroed here.
static inline void rgcn_fill_occupancy(const int32_t* rowptr, int64_t n_key, int64_t R, uint32_t* words) {
  const int64_t off = rgcn_row_mask_offset(n_key), total = rgcn_occupancy_words(n_key);
  for (int64_t i = 0; i < total; ++i) words[i] = 0u;
  for (int64_t i = 0; i < n_key; ++i) {
    uint32_t m = 0u;
    for (int64_t r = 0; r < R; ++r)
      if (rowptr[i * R + r + 1] > rowptr[i * R + r]) m |= 1u << r;
    words[off + i] = m;
    words[i >> 5] |= m;
  }
}

// The occupancy ORDER of the rows (include/rgcn_row_order.h), behind the pad words of the same allocation - reachable,
// like the row words, from tile_mask and the row count alone: rows grouped by their occupancy word, groups with more
// relations first, natural order inside a group.  The split NT transforms take their 64-row tiles in that order
// (RGCN_MODE_ROW_ORDER), so that a tile's relation word is (nearly always) every row's word and the k-tiles of the
// other relations are skipped: 50 % of C2's (tile, relation) blocks are live then, against 75 % in node order.
struct rgcn_order_offsets {
  int64_t P, perm, rows, tiles, fin, items;      // padded rows; word offsets of the sections (each a multiple of 4)
};
static inline rgcn_order_offsets rgcn_order_offsets_of(int64_t n_key) {
  rgcn_order_offsets o;
  o.P = (n_key + 63) / 64 * 64;
  const int64_t t32 = o.P / 32;
  o.perm = (rgcn_occupancy_words(n_key) + 3) / 4 * 4;
  o.rows = o.perm + o.P;
  o.tiles = o.rows + o.P;
  o.fin = o.tiles + (t32 + 3) / 4 * 4;
  o.items = o.fin + (t32 + 1 + 3) / 4 * 4;
  return o;
}
// Host side: `words` holds the occupancy words (rgcn_fill_occupancy) and grows by the order.  `level1`: the items of
// a single reduce level (deferred hub tails), in plan order, or none.
static inline void rgcn_fill_row_order(int64_t n_key, int64_t R, const rgcn_item* level1, int64_t num_level1,
                                       std::vector<uint32_t>& words) {
  const rgcn_order_offsets o = rgcn_order_offsets_of(n_key);
  const uint32_t* row = words.data() + rgcn_row_mask_offset(n_key);
  std::vector<uint64_t> key((size_t)n_key);
  std::vector<int32_t> perm((size_t)n_key), pos((size_t)n_key);
  for (int64_t i = 0; i < n_key; ++i) {
    key[(size_t)i] = ((uint64_t)(32 - __builtin_popcount(row[i])) << 32) | row[i];
    perm[(size_t)i] = (int32_t)i;
  }
  std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
  for (int64_t p = 0; p < n_key; ++p) pos[(size_t)perm[(size_t)p]] = (int32_t)p;
  words.resize((size_t)(o.items + 4 * num_level1), 0u);
  row = words.data() + rgcn_row_mask_offset(n_key);              // (the vector may have moved)
  for (int64_t p = 0; p < o.P; ++p) {
    const int32_t src = perm[(size_t)(p < n_key ? p : n_key - 1)];
    const uint32_t m = p < n_key ? row[src] : 0u;
    words[(size_t)(o.perm + p)] = (uint32_t)src;
    words[(size_t)(o.rows + p)] = m;
    words[(size_t)(o.tiles + (p >> 5))] |= m;
  }
  if (num_level1 > 0) {
    const int64_t t32 = o.P / 32;
    auto tile_of = [&](const rgcn_item& it) { return (int64_t)(pos[(size_t)(it.dst / R)] >> 5); };
    std::vector<rgcn_item> items(level1, level1 + num_level1);
    std::stable_sort(items.begin(), items.end(), [&](const rgcn_item& a, const rgcn_item& b) { return tile_of(a) < tile_of(b); });
    uint32_t* fin = words.data() + o.fin;
    for (const rgcn_item& it : items) ++fin[tile_of(it) + 1];
    for (int64_t t = 0; t < t32; ++t) fin[t + 1] += fin[t];
    for (int64_t j = 0; j < num_level1; ++j) {
      const rgcn_item& it = items[(size_t)j];
      uint32_t* w = words.data() + o.items + 4 * j;
      w[0] = (uint32_t)it.begin; w[1] = (uint32_t)it.end; w[2] = (uint32_t)it.dst; w[3] = (uint32_t)it.flags;
    }
  }
}

struct rgcn_graph {
  int64_t E = 0, N = 0, R = 0;
  rgcn_csr dir[2];  // [0] forward (dst,rel), [1] transposed (src,rel)
};

// Device address of the current device's sticky index-error flag (distmult.hip; rgcn_index_error_fetch reads and
// clears it) for the kernels that meet an id outside its table: they take it as a parameter.  NULL if HIP fails.
// The address is looked up on the first call per device and kept.  That lookup is not a stream operation, so a call
// that is being captured into a HIP graph must not make it: an eager call on the device comes first.
__attribute__((visibility("hidden"))) int* rgcn_index_error_flag();

// rgcn_aggregate_ex with RGCN_MODE_WEIGHT_GRAD in its option word (edge_grad.hip): the same parameters in the roles
// include/rgcn_hip.h gives them there - `gagg` is the call's agg, `out` / `out_bytes` its workspace.  g is not NULL.
__attribute__((visibility("hidden"))) int rgcn_edge_grad(const rgcn_graph* g, int transposed, const void* x, int mode,
                                                         int64_t d, const float* gagg, void* out, size_t out_bytes,
                                                         int first_level, int last_level, const rgcn_slab_job* job,
                                                         const float* amax, void* stream);
// ... with RGCN_MODE_EDGE_SUM (edge_grad.hip): `x` is float[E] by original column, `out` the call's agg.  g is not NULL.
__attribute__((visibility("hidden"))) int rgcn_edge_sum(const rgcn_graph* g, int transposed, const void* x, int mode,
                                                        int64_t d, float* out, int first_level, int last_level,
                                                        const rgcn_slab_job* job, const float* amax, void* stream);

// ---------------------------------------------------------------------------------------------
// "amax" buffers: max |tensor| as the split-precision transforms need it (rgcn_transform_split.hip).
// A buffer is RGCN_AMAX_FLOATS floats, zeroed by the caller; its VALUE is the maximum over all entries.
// Producers publish wave maxima into one of RGCN_AMAX_SLOTS slots, 128 bytes apart (own cache lines, so
// the integer atomics of a launch spread over L2 channels instead of queueing on one address - 50k
// same-address atomics cost a gather launch 10x its time), chosen by workgroup id, and only when the
// wave's maximum exceeds what the slot already shows (a stale read is safe: slots only grow).  The bit
// pattern of a non-negative float orders like an unsigned int and a maximum does not depend on arrival
// order, so the value is run-to-run deterministic.
// ---------------------------------------------------------------------------------------------
constexpr int RGCN_AMAX_SLOTS = 64, RGCN_AMAX_STRIDE = 32;
// Heads = the entries that are ever written: RGCN_AMAX_HEADS of them, RGCN_AMAX_HEAD_STRIDE floats apart.  The
// scan kernel (rgcn_absmax) writes one partial maximum per workgroup into every head without atomics; the
// publishing slots above are every fourth head.  A buffer's value is the maximum over its heads.
constexpr int RGCN_AMAX_HEADS = 256, RGCN_AMAX_HEAD_STRIDE = 8;
static_assert(RGCN_AMAX_SLOTS * RGCN_AMAX_STRIDE == RGCN_AMAX_FLOATS, "amax buffer layout (include/rgcn_hip.h)");
static_assert(RGCN_AMAX_HEADS * RGCN_AMAX_HEAD_STRIDE == RGCN_AMAX_FLOATS && RGCN_AMAX_STRIDE % RGCN_AMAX_HEAD_STRIDE == 0,
              "amax buffer layout");

#if defined(__HIPCC__)
// v held to [lo, hi]: the bounds of a CSR row read from memory that may be damaged
__device__ inline int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
// lane src's value of v as a wave-uniform (scalar) value
__device__ inline int lane_int(int v, int src) { return __builtin_amdgcn_readfirstlane(__shfl(v, src)); }
__device__ inline float lane_float(float v, int src) { return __int_as_float(lane_int(__float_as_int(v), src)); }
__device__ inline int64_t lane_i64(int64_t v, int src) {
  const unsigned lo = (unsigned)lane_int((int)(unsigned)(v & 0xffffffffll), src);
  const int hi = lane_int((int)(v >> 32), src);
  return ((int64_t)hi << 32) | (int64_t)lo;
}
// The ReLU of every fused epilogue.  fmaxf returns its non-NaN operand, so fmaxf(NaN, 0) is 0 and a diverged
// pre-activation would leave the layer looking healthy; torch.relu(NaN) is NaN.  The select puts the NaN back and
// leaves every other input with the bits fmaxf(v, 0.f) gives it (-0 included; +inf stays +inf, -inf becomes 0).
__device__ inline float rgcn_relu(float v) {
  const float r = fmaxf(v, 0.f);
  return v != v ? v : r;
}
extern "C" __device__ unsigned __ockl_wfred_max_u32(unsigned);
// Called by lanes 0 .. k of a wave, for any k (a last wave that is not full) - NOT by a subset with holes: the DPP
// reduction behind __ockl_wfred_max_u32 gathers a row of 16 lanes in the row's lane 0 and hands rows 1 and 3 on
// through lanes 15 and 47, so a maximum held by a row whose lane 0, or whose neighbour's lane 15, has left is lost
// (the gather at d = 4 published 1.64 for rows whose maximum was 7).  Lanes with nothing to report pass 0.
// `seen`: what the slot showed when the wave started (rgcn_amax_peek) - read early so that the tail of a
// wave does not wait for a dependent load; a stale value only costs an atomic that changes nothing
__device__ inline unsigned rgcn_amax_peek(const unsigned* __restrict__ amax) {
  return amax ? amax[(blockIdx.x & (RGCN_AMAX_SLOTS - 1)) * RGCN_AMAX_STRIDE] : 0u;
}
// A lane whose values were all NaN arrives with a NaN maximum (fmaxf(NaN, NaN)); its bit pattern would win the integer
// max and poison the buffer, so it reports 0 like a lane with nothing to report: a published maximum is never NaN.
__device__ inline void rgcn_amax_publish(unsigned* __restrict__ amax, float lane_max, unsigned seen = 0u) {
  const unsigned m = __ockl_wfred_max_u32(__float_as_uint(fmaxf(lane_max, 0.f)));
  if (m <= seen) return;
  unsigned* slot = amax + (blockIdx.x & (RGCN_AMAX_SLOTS - 1)) * RGCN_AMAX_STRIDE;
  const unsigned long long act = __ballot(1);
  if ((int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicMax(slot, m);
}
// the buffer's value, by every lane of a wave: four independent loads per lane (only the heads are ever written)
__device__ inline float rgcn_amax_value(const float* __restrict__ amax, int lane) {
  float v[RGCN_AMAX_HEADS / 64];
#pragma unroll
  for (int j = 0; j < RGCN_AMAX_HEADS / 64; ++j) v[j] = amax[(lane + 64 * j) * RGCN_AMAX_HEAD_STRIDE];
  float m = v[0];
#pragma unroll
  for (int j = 1; j < RGCN_AMAX_HEADS / 64; ++j) m = fmaxf(m, v[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  return m;
}
// max of `count` <= 256 contiguous partials, by every lane of a wave: four independent loads per lane
__device__ inline float rgcn_partials_max(const float* __restrict__ p, int count, int lane) {
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (lane + 64 * j < count) ? p[lane + 64 * j] : 0.f;
  float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  return m;
}
#endif
