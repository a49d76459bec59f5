// Device-side mini-batch assembly with type-constrained, filtered negatives (include/rgcn_sampling.h).
//
// sampler.hip draws every replacement uniformly over all nodes and never looks at the graph, so most
// negatives are of the wrong node type and a few are known triples labelled 0.  This launch is the same
// one-thread-per-sample assembly with the evaluation protocol's two structures consulted on the device:
// the class index of ops.NodeClasses and the two CSRs of ops.KnownTriples.
//
// Contract (restated on the host by tests/test_sampler_constrained*.py):
//   - Positives, relations, labels, the clamping of a window past the end and ctr = (cursor + p) * k + j
//     are exactly the plain sampler's.
//   - Block t, t = 0 .. T-1, is Philox4x32-10 with key = the two halves of the seed and counter
//     (ctr_lo, ctr_hi, epoch_lo, epoch_hi XOR (t << 24)).  Block 0 is the plain sampler's block.  Epochs
//     must stay below 2^56 (bits 56..59 of the epoch carry the try).
//   - Side: top bit of word 0 of block 0.  Set: the head is replaced, the anchor is the tail, the known side
//     is "head".  Clear: the tail is replaced, the anchor is the head, the known side is "tail".
//   - Candidate of try t, w = word 1 of block t.  No classes: (w * N) >> 32.  With classes, c =
//     class_of[replaced node]: c < 0 or class c empty -> (w * N) >> 32, otherwise
//     class_members[class_ptr[c] + ((w * size_c) >> 32)].
//   - The first accepted candidate wins.  Accepted: no known set given, or (anchor, relation, candidate) not
//     in it - a binary search of keys for anchor * R + relation, then one of that segment's ids.  Every
//     rejected draw adds 1 to stats[0].
//   - All T draws rejected: the last candidate is kept and stats[1] gains 1.
//   - All three groups null and T = 1: the output equals rgcn_sample_batch bit for bit.
//
// Memory safety does not rest on the inputs being well formed: positions and columns are clamped as in the
// plain sampler, a replaced node outside [0, N) has no class, a class id >= C or a class range outside the
// member array is treated as "no class", an anchor or relation outside its range is in no known triple
// (it must not alias another anchor's key), and segment bounds are clamped to the id array.
#include "rgcn_common.h"
#include "../../include/rgcn_sampling.h"
#include "rgcn_sample_core.h"
#include "rgcn_sorted_search.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTries = 16;

struct known_side {
  const int64_t* keys;
  const int64_t* ptr;
  const int64_t* ids;
  int64_t num_keys, nnz;
};

struct sample_args {
  const int64_t* edge_index;
  const int64_t* edge_type;
  int64_t E;
  const int64_t* order;
  const int64_t* cursor;
  int64_t B, k, num_nodes;
  const int64_t* rng;
  const int32_t* class_of;         // null: no classes
  const int64_t* class_ptr;
  const int64_t* class_members;
  int64_t num_classes;
  known_side side[2];              // [0] "tail", [1] "head"; keys null: no known set
  int64_t num_relations;
  int tries;
  unsigned long long* stats;       // null: not counted
  int64_t* heads;
  int64_t* tails;
  int64_t* rels;
  float* labels;
};

__device__ inline int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kThreads) void k_sample_batch_constrained(const sample_args a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t B = a.B, k = a.k, E = a.E, N = a.num_nodes;
  const bool live = i < B * (1 + k);         // no early return: every lane takes part in the wave sums below
  int rejected = 0, gave_up = 0;
  if (live) {
    const rgcn_positive s = rgcn_sample_positive(a.edge_index, E, a.order, a.cursor, B, k, i);
    int64_t h = s.h, t = s.t;
    const int64_t rel = a.edge_type[s.colm];
    if (i >= B) {
      const uint32_t k0 = (uint32_t)a.rng[0], k1 = (uint32_t)((uint64_t)a.rng[0] >> 32);
      const uint32_t e0 = (uint32_t)a.rng[1], e1 = (uint32_t)((uint64_t)a.rng[1] >> 32);
      const uint64_t ctr = rgcn_sample_counter(s.start, B, k, i);
      uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), e0, e1};
      philox4x32_10(c, k0, k1);
      const bool replace_head = (c[0] >> 31) != 0;
      const int64_t replaced = replace_head ? h : t, anchor = replace_head ? t : h;
      // where the candidates come from: the members of the replaced node's class, or all nodes
      int64_t base = -1, range = N;
      if (a.class_of && replaced >= 0 && replaced < N) {
        const int64_t cls = a.class_of[replaced];
        if (cls >= 0 && cls < a.num_classes) {
          const int64_t lo = a.class_ptr[cls], hi = a.class_ptr[cls + 1];
          if (lo >= 0 && hi > lo && hi <= a.class_ptr[a.num_classes]) {
            base = lo;
            range = hi - lo;
          }
        }
      }
      // the segment of (anchor, relation) in the known side: [seg_lo, seg_hi) of ids, empty if nothing is known
      const known_side ks = replace_head ? a.side[1] : a.side[0];
      int64_t seg_lo = 0, seg_hi = 0;
      if (ks.keys && anchor >= 0 && anchor < N && rel >= 0 && rel < a.num_relations) {
        const int64_t key = anchor * a.num_relations + rel;
        const int64_t at = rgcn_lower_bound(ks.keys, 0, ks.num_keys, key);
        if (at < ks.num_keys && ks.keys[at] == key) {
          seg_lo = ks.ptr[at];
          seg_hi = ks.ptr[at + 1];
          seg_lo = seg_lo < 0 ? 0 : (seg_lo > ks.nnz ? ks.nnz : seg_lo);
          seg_hi = seg_hi < seg_lo ? seg_lo : (seg_hi > ks.nnz ? ks.nnz : seg_hi);
        }
      }
      int64_t entity = 0;
      for (int tr = 0; tr < a.tries; ++tr) {
        if (tr > 0) {                          // block tr: the same counter with the try in the top epoch bits
          c[0] = (uint32_t)ctr; c[1] = (uint32_t)(ctr >> 32); c[2] = e0; c[3] = e1 ^ ((uint32_t)tr << 24);
          philox4x32_10(c, k0, k1);
        }
        const int64_t draw = rgcn_sample_draw(c[1], range);
        entity = base < 0 ? draw : a.class_members[base + draw];
        bool known = false;
        if (seg_hi > seg_lo) {
          const int64_t at = rgcn_lower_bound(ks.ids, seg_lo, seg_hi, entity);
          known = at < seg_hi && ks.ids[at] == entity;
        }
        if (!known) break;
        ++rejected;
        if (tr + 1 == a.tries) gave_up = 1;
      }
      if (replace_head) h = entity; else t = entity;
    }
    a.heads[i] = h;
    a.tails[i] = t;
    a.rels[i] = rel;
    a.labels[i] = i < B ? 1.f : 0.f;
  }
  if (a.stats) {                               // uniform over the launch: all 64 lanes of every wave arrive here
    const int r = wave_sum(rejected), g = wave_sum(gave_up);
    if ((threadIdx.x & 63) == 0) {
      if (r) atomicAdd(a.stats, (unsigned long long)r);
      if (g) atomicAdd(a.stats + 1, (unsigned long long)g);
    }
  }
}

}  // namespace

extern "C" int rgcn_sample_batch_constrained(
    const int64_t* edge_index, const int64_t* edge_type, int64_t num_edges, const int64_t* order, const int64_t* cursor,
    int64_t batch, int64_t num_neg, int64_t num_nodes, const int64_t* rng, const int32_t* class_of,
    const int64_t* class_ptr, const int64_t* class_members, int64_t num_classes, const int64_t* tail_keys,
    const int64_t* tail_ptr, const int64_t* tail_ids, int64_t tail_num_keys, int64_t tail_nnz, const int64_t* head_keys,
    const int64_t* head_ptr, const int64_t* head_ids, int64_t head_num_keys, int64_t head_nnz, int64_t num_relations,
    int max_tries, int64_t* stats, int64_t* heads, int64_t* tails, int64_t* rels, float* labels, void* stream_) {
  if (batch < 0 || num_neg < 0 || num_edges < 0 || num_nodes <= 0) return RGCN_ERR_ARG;
  if (max_tries < 1 || max_tries > kMaxTries) return RGCN_ERR_ARG;
  // a group is given whole or not at all
  const int class_given = (class_of != nullptr) + (class_ptr != nullptr) + (class_members != nullptr);
  if (class_given != 0 && (class_given != 3 || num_classes <= 0)) return RGCN_ERR_ARG;
  const int known_given = (tail_keys != nullptr) + (tail_ptr != nullptr) + (tail_ids != nullptr) +
                          (head_keys != nullptr) + (head_ptr != nullptr) + (head_ids != nullptr);
  if (known_given != 0 && (known_given != 6 || num_relations <= 0 || tail_num_keys <= 0 || tail_nnz <= 0 ||
                           head_num_keys <= 0 || head_nnz <= 0))
    return RGCN_ERR_ARG;
  if (num_nodes > ((int64_t)1 << 32)) return RGCN_ERR_UNSUPPORTED;
  const int64_t total = batch * (1 + num_neg);
  if (total == 0) return RGCN_OK;
  if (num_edges == 0 || !edge_index || !edge_type || !heads || !tails || !rels || !labels) return RGCN_ERR_ARG;
  if (num_neg > 0 && !rng) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(8, edge_index, edge_type, order, cursor, rng, class_ptr, class_members, tail_keys, tail_ptr, tail_ids,
                 head_keys, head_ptr, head_ids, stats, heads, tails, rels);
  RGCN_ALIGN_TRY(4, class_of, labels);
  sample_args a;
  a.edge_index = edge_index; a.edge_type = edge_type; a.E = num_edges; a.order = order; a.cursor = cursor;
  a.B = batch; a.k = num_neg; a.num_nodes = num_nodes; a.rng = rng;
  a.class_of = class_of; a.class_ptr = class_ptr; a.class_members = class_members; a.num_classes = num_classes;
  a.side[0] = {tail_keys, tail_ptr, tail_ids, tail_num_keys, tail_nnz};
  a.side[1] = {head_keys, head_ptr, head_ids, head_num_keys, head_nnz};
  a.num_relations = num_relations; a.tries = max_tries; a.stats = (unsigned long long*)stats;
  a.heads = heads; a.tails = tails; a.rels = rels; a.labels = labels;
  hipStream_t stream = (hipStream_t)stream_;
  k_sample_batch_constrained<<<(unsigned)ceil_div64(total, kThreads), kThreads, 0, stream>>>(a);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}
