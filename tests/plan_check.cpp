// Stand-alone check of the gather's work plan (csrc/rgcn_plan.h, the host code rgcn_graph.hip uploads), meant to run
// under AddressSanitizer / UndefinedBehaviorSanitizer.  Every input rowptr is planned and the plan is EXECUTED
// symbolically in integers: edge e is worth a 64-bit hash of e, a level-0 item sums its edges, a pack leader adds its
// members, a reduce item sums the partial rows it names - and then
//   level 0   : every edge index is covered exactly once; an item has at most RGCN_CHUNK edges; packs sit in
//               RGCN_PACK-aligned, consecutive slots (leader, members, SKIP padding) with follower count = runs - 1 and
//               the MEMBER / SKIP / FINAL flags as rgcn_plan.h documents them; packs come before singles, each by
//               descending length, stable;
//   levels>=1 : an item has 1 .. RGCN_CHUNK_UP rows and reads only rows a LOWER level wrote; every partial row is
//               written exactly once and read exactly once; num_partials = highest row + 1;
//   segments  : every segment, empty ones included, receives exactly one FINAL write, worth the sum of its edges;
//   fin_ptr   : present iff the plan has exactly two levels; non-decreasing, covers level 1, and the items of
//               [fin_ptr[t], fin_ptr[t + 1]) have (dst / R) >> 5 == t.
// Inputs: single segments at the level thresholds (131,072 / 131,073 / 262,444 / 67,108,864 / 67,108,865) with the
// plan sizes written out, the run / pack boundaries, seeded random rowptrs with hubs of two and three levels, and -
// with --full - the top of the int32 range, where the cuts `begin + (p + 1) * span` do not fit an int32.
// The plans of all inputs but the top of the range are also held, as FNV-1a digests, to the plans the planner gave
// before it moved into the header (kParentDigest below).
#include <sys/resource.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "primekg_rgcn_linkprediction_amd/csrc/rgcn_plan.h"

#define FAIL(...)                                  \
  do {                                             \
    std::printf("plan_check FAILED [%s]: ", name); \
    std::printf(__VA_ARGS__);                      \
    std::printf("\n");                             \
    std::exit(1);                                  \
  } while (0)

static inline uint64_t edge_value(int64_t e) {          // splitmix64 finalizer
  uint64_t z = (uint64_t)e + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint64_t range_value(int64_t b, int64_t e) {
  uint64_t s = 0;
  for (int64_t i = b; i < e; ++i) s += edge_value(i);
  return s;
}

static void fnv(uint64_t& h, const void* p, size_t n) {
  const unsigned char* c = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) {
    h ^= c[i];
    h *= 0x100000001B3ull;
  }
}
static void fnv64(uint64_t& h, int64_t v) { fnv(h, &v, sizeof v); }

struct Shape {
  int levels = 0;
  int64_t partials = 0;
  std::vector<int64_t> items;
};

// plans rowptr, checks everything listed above, returns the digest of the plan
static uint64_t check_case(const char* name, const std::vector<int32_t>& rowptr, int64_t n_key, int64_t R, Shape* shape) {
  const int64_t NR = n_key * R;
  if ((int64_t)rowptr.size() != NR + 1) FAIL("rowptr has %zu entries for NR = %lld", rowptr.size(), (long long)NR);
  const int64_t E = rowptr[(size_t)NR];
  rgcn_plan plan;
  const int rc = rgcn_build_plan(rowptr, NR, R, n_key, &plan);
  if (rc != RGCN_OK) FAIL("rgcn_build_plan returned %d", rc);
  const auto& levels = plan.levels;
  const int nl = (int)levels.size();
  if (nl < 1 || nl > RGCN_MAX_LEVELS) FAIL("%d levels", nl);
  const int64_t P = plan.num_partials;
  if (P < 0 || P > INT32_MAX) FAIL("num_partials %lld", (long long)P);

  std::vector<uint64_t> pval((size_t)P, 0), fval((size_t)NR, 0);
  std::vector<int8_t> plevel((size_t)P, -1);             // level that wrote the row
  std::vector<uint8_t> pread((size_t)P, 0), fwrites((size_t)NR, 0);
  int64_t highest = -1;
  auto write_row = [&](const rgcn_item& it, uint64_t v, int level, int64_t at) {
    if (it.flags & RGCN_ITEM_FINAL) {
      if (it.dst < 0 || it.dst >= NR) FAIL("level %d item %lld: final row %d outside [0, %lld)", level, (long long)at, it.dst, (long long)NR);
      if (fwrites[(size_t)it.dst]++) FAIL("segment %d receives a second FINAL write (level %d item %lld)", it.dst, level, (long long)at);
      fval[(size_t)it.dst] = v;
    } else {
      if (it.dst < 0 || it.dst >= P) FAIL("level %d item %lld: partial row %d outside [0, %lld)", level, (long long)at, it.dst, (long long)P);
      if (plevel[(size_t)it.dst] >= 0) FAIL("partial row %d is written twice (level %d item %lld)", it.dst, level, (long long)at);
      plevel[(size_t)it.dst] = (int8_t)level;
      pval[(size_t)it.dst] = v;
      highest = std::max<int64_t>(highest, it.dst);
    }
  };

  // ---- level 0
  {
    const auto& L0 = levels[0];
    const int64_t n0 = (int64_t)L0.size();
    std::vector<uint64_t> cover;                          // (begin << 32 | end) of every non-empty run
    cover.reserve((size_t)n0);
    int64_t i = 0, prev_len = INT64_MAX, prev_begin = -1;
    while (i < n0 && (L0[(size_t)i].flags & RGCN_ITEM_PACK)) {      // packs: whole groups of RGCN_PACK slots
      if (i % RGCN_PACK) FAIL("pack at slot %lld is not aligned", (long long)i);
      if (i + RGCN_PACK > n0) FAIL("the last pack is short of slots");
      const rgcn_item& lead = L0[(size_t)i];
      if (lead.flags & (RGCN_ITEM_MEMBER | RGCN_ITEM_SKIP)) FAIL("slot %lld: a pack starts with a member or padding", (long long)i);
      if (lead.flags & ~(RGCN_ITEM_PACK | RGCN_ITEM_FINAL | ((RGCN_PACK - 1) << RGCN_ITEM_FOLLOW_SHIFT)))
        FAIL("slot %lld: unknown flag bits %x", (long long)i, lead.flags);
      const int followers = (lead.flags >> RGCN_ITEM_FOLLOW_SHIFT) & (RGCN_PACK - 1);
      uint64_t v = 0;
      int64_t at = lead.begin;
      for (int c = 0; c < RGCN_PACK; ++c) {
        const rgcn_item& it = L0[(size_t)(i + c)];
        if (c > followers) {
          if (it.flags != (RGCN_ITEM_PACK | RGCN_ITEM_SKIP) || it.begin != 0 || it.end != 0 || it.dst != 0)
            FAIL("slot %lld: padding of a pack is {%d, %d, %d, %x}", (long long)(i + c), it.begin, it.end, it.dst, it.flags);
          continue;
        }
        if (c > 0 && it.flags != (RGCN_ITEM_PACK | RGCN_ITEM_MEMBER)) FAIL("slot %lld: member flags %x", (long long)(i + c), it.flags);
        if (it.dst != lead.dst) FAIL("slot %lld: member names row %d, its leader %d", (long long)(i + c), it.dst, lead.dst);
        const int64_t len = (int64_t)it.end - it.begin;
        if (it.begin != at || it.begin < 0) FAIL("slot %lld: run begins at %d, the one before ended at %lld", (long long)(i + c), it.begin, (long long)at);
        if (len < 1 || len > RGCN_CHUNK || (c < followers && len != RGCN_CHUNK))          // followers = runs - 1
          FAIL("slot %lld: run %d of %d has %lld edges", (long long)(i + c), c, followers + 1, (long long)len);
        if (it.end > E) FAIL("slot %lld: run ends at %d past E = %lld", (long long)(i + c), it.end, (long long)E);
        at = it.end;
        v += range_value(it.begin, it.end);
        cover.push_back(((uint64_t)(uint32_t)it.begin << 32) | (uint32_t)it.end);
      }
      const int64_t plen = at - lead.begin;
      if ((lead.flags & RGCN_ITEM_FINAL) && plen <= RGCN_CHUNK) FAIL("slot %lld: a whole segment of %lld edges as a pack", (long long)i, (long long)plen);
      if (plen > prev_len || (plen == prev_len && lead.begin <= prev_begin))
        FAIL("slot %lld: packs are not by descending length, stable", (long long)i);
      prev_len = plen;
      prev_begin = lead.begin;
      if ((lead.flags & RGCN_ITEM_FINAL) &&
          (lead.dst < 0 || lead.dst >= NR || lead.begin != rowptr[(size_t)lead.dst] || at != rowptr[(size_t)lead.dst + 1]))
        FAIL("slot %lld: a FINAL pack is not its whole segment", (long long)i);
      write_row(lead, v, 0, i);
      i += RGCN_PACK;
    }
    prev_len = INT64_MAX;
    int64_t prev_dst = -1;
    for (; i < n0; ++i) {                                  // singles
      const rgcn_item& it = L0[(size_t)i];
      if (it.flags != RGCN_ITEM_FINAL) FAIL("slot %lld: flags %x behind the packs", (long long)i, it.flags);
      const int64_t len = (int64_t)it.end - it.begin;
      if (len < 0 || len > RGCN_CHUNK) FAIL("slot %lld: single item of %lld edges", (long long)i, (long long)len);
      if (it.dst < 0 || it.dst >= NR || it.begin != rowptr[(size_t)it.dst] || it.end != rowptr[(size_t)it.dst + 1])
        FAIL("slot %lld: a single item is not its whole segment", (long long)i);
      if (len > prev_len || (len == prev_len && it.dst <= prev_dst)) FAIL("slot %lld: singles are not by descending length, stable", (long long)i);
      prev_len = len;
      prev_dst = it.dst;
      if (len > 0) cover.push_back(((uint64_t)(uint32_t)it.begin << 32) | (uint32_t)it.end);
      write_row(it, range_value(it.begin, it.end), 0, i);
    }
    std::sort(cover.begin(), cover.end());
    int64_t at = 0;
    for (uint64_t c : cover) {
      if ((int64_t)(c >> 32) != at) FAIL("edge %lld is covered %s", (long long)at, (int64_t)(c >> 32) > at ? "by no item" : "twice");
      at = (int64_t)(uint32_t)c;
    }
    if (at != E) FAIL("edges [%lld, %lld) are covered by no item", (long long)at, (long long)E);
  }

  // ---- reduce levels
  for (int l = 1; l < nl; ++l) {
    if (levels[(size_t)l].empty()) FAIL("level %d is empty", l);
    int64_t at = 0;
    for (const rgcn_item& it : levels[(size_t)l]) {
      const int64_t len = (int64_t)it.end - it.begin;
      if (it.flags & ~RGCN_ITEM_FINAL) FAIL("level %d item %lld: flags %x", l, (long long)at, it.flags);
      if (len < 1 || len > RGCN_CHUNK_UP || it.begin < 0 || it.end > P) FAIL("level %d item %lld: rows [%d, %d)", l, (long long)at, it.begin, it.end);
      uint64_t v = 0;
      for (int32_t r = it.begin; r < it.end; ++r) {
        if (plevel[(size_t)r] < 0 || plevel[(size_t)r] >= l) FAIL("level %d item %lld reads row %d, written by level %d", l, (long long)at, r, plevel[(size_t)r]);
        if (pread[(size_t)r]++) FAIL("partial row %d is read twice (level %d item %lld)", r, l, (long long)at);
        v += pval[(size_t)r];
      }
      write_row(it, v, l, at);
      ++at;
    }
  }
  for (int64_t r = 0; r < P; ++r)
    if (plevel[(size_t)r] < 0 || pread[(size_t)r] != 1) FAIL("partial row %lld: written by level %d, read %d times", (long long)r, plevel[(size_t)r], pread[(size_t)r]);
  if (P != highest + 1) FAIL("num_partials %lld, highest row %lld", (long long)P, (long long)highest);
  for (int64_t s = 0; s < NR; ++s) {
    if (fwrites[(size_t)s] != 1) FAIL("segment %lld receives no FINAL write", (long long)s);
    if (fval[(size_t)s] != range_value(rowptr[(size_t)s], rowptr[(size_t)s + 1])) FAIL("segment %lld: the plan's sum is not the sum of its edges", (long long)s);
  }

  // ---- fin_ptr
  const auto& fp = plan.fin_ptr;
  if ((nl == 2) != !fp.empty()) FAIL("%d levels, fin_ptr of %zu entries", nl, fp.size());
  if (!fp.empty()) {
    const int64_t tiles = ceil_div64(n_key, 32);
    if ((int64_t)fp.size() != tiles + 1 || fp[0] != 0 || fp[(size_t)tiles] != (int64_t)levels[1].size()) FAIL("fin_ptr does not cover level 1");
    for (int64_t t = 0; t < tiles; ++t) {
      if (fp[(size_t)t + 1] < fp[(size_t)t]) FAIL("fin_ptr decreases at tile %lld", (long long)t);
      for (int32_t k = fp[(size_t)t]; k < fp[(size_t)t + 1]; ++k)
        if (((int64_t)(levels[1][(size_t)k].dst / R) >> 5) != t) FAIL("level-1 item %d is filed under tile %lld", k, (long long)t);
    }
  }

  uint64_t h = 0xCBF29CE484222325ull;
  fnv64(h, nl);
  for (const auto& v : levels) {
    fnv64(h, (int64_t)v.size());
    if (!v.empty()) fnv(h, v.data(), v.size() * sizeof(rgcn_item));
  }
  fnv64(h, (int64_t)fp.size());
  if (!fp.empty()) fnv(h, fp.data(), fp.size() * sizeof(int32_t));
  fnv64(h, P);
  shape->levels = nl;
  shape->partials = P;
  shape->items.clear();
  for (const auto& v : levels) shape->items.push_back((int64_t)v.size());
  return h;
}

struct Rng {                                              // splitmix64: the same stream with every standard library
  uint64_t s;
  uint64_t next() { return edge_value((int64_t)(s++)); }
  int64_t below(int64_t n) { return (int64_t)(next() % (uint64_t)n); }
};

// n_key nodes x R relations: empty segments at both ends, short segments of every kind, `hubs2` segments with one
// reduce level and `hubs3` with two
static std::vector<int32_t> random_rowptr(uint64_t seed, int64_t n_key, int64_t R, int hubs2, int hubs3) {
  Rng g{seed * 0x1000003ull + 17};
  const int64_t NR = n_key * R;
  std::vector<int64_t> len((size_t)NR, 0);
  const int64_t lead = 1 + g.below(40), trail = 1 + g.below(40);
  for (int64_t s = lead; s < NR - trail; ++s) {
    const int64_t kind = g.below(16);
    if (kind < 4) len[(size_t)s] = 0;
    else if (kind < 10) len[(size_t)s] = g.below(RGCN_CHUNK + 2);
    else if (kind < 13) len[(size_t)s] = 60 + g.below(12) + RGCN_CHUNK * g.below(5);
    else if (kind < 15) len[(size_t)s] = 250 + g.below(14) + 256 * g.below(4);
    else len[(size_t)s] = 1 + g.below(3000);
  }
  for (int k = 0; k < hubs2 + hubs3; ++k) {
    const int64_t s = lead + g.below(NR - lead - trail);
    len[(size_t)s] = k < hubs2 ? 257 + g.below(131072 - 256) : 131073 + g.below(400000);
  }
  std::vector<int32_t> rowptr((size_t)NR + 1, 0);
  for (int64_t s = 0; s < NR; ++s) rowptr[(size_t)s + 1] = (int32_t)(rowptr[(size_t)s] + len[(size_t)s]);
  return rowptr;
}

// Plans of the fixed inputs as the parent of the commit that moved the planner into rgcn_plan.h gave them
// (564229c: the body of build_plan in csrc/rgcn_graph.hip, copied verbatim into a scratch program that ran this file's
// inputs and digest).  The top-of-range inputs are not among them: that build_plan overflows there.
static const uint64_t kParentDigest[] = {
    0x218B92DE6EF8DE96ull,
    0x29CAE3F870ADE5EAull,
    0x668232E8F2930B93ull,
    0xFFD049759C2CD844ull,
    0x7A3E20C06213E4D9ull,
    0x141336A7134C7FF4ull,
    0x81ABA9C9368974A5ull,
    0xC4545F325FCBBC34ull,
    0x3595D1A592C1F5BFull,
    0x72ABADED6F1BC02Full,
    0x8C6D9DB3919CC916ull,
    0x23DC6062A056C387ull,
    0x9AD0521872D31343ull,
    0xB7D1E67CCF4A7FFCull,
    0xCF477AF86E74467Aull,
    0x4D2116D406118162ull,
    0x752C0AFC3D300F64ull,
    0x65D76660D71551FCull,
    0x35ECC2E572CAEEE2ull,
    0x1C501C1093FC2E52ull,
};

int main(int argc, char** argv) {
  const bool full = argc > 1 && std::strcmp(argv[1], "--full") == 0;
  const bool print_digests = argc > 1 && std::strcmp(argv[1], "--digests") == 0;
  struct Fixed { const char* name; int64_t len; int levels; int64_t partials; std::vector<int64_t> items; };
  const std::vector<Fixed> singles = {
      {"131072", 131072, 2, 512, {2048, 1}},
      {"131073", 131073, 3, 515, {2052, 2, 1}},
      {"262444", 262444, 3, 1029, {4104, 3, 1}},
      {"67108864", 67108864, 3, 262656, {1048576, 512, 1}},
      {"67108865", 67108865, 4, 262660, {1048580, 513, 2, 1}},
      {"0", 0, 1, 0, {1}},
      {"1", 1, 1, 0, {1}},
      {"64", 64, 1, 0, {1}},
      {"65", 65, 1, 0, {4}},
      {"256", 256, 1, 0, {4}},
      {"257", 257, 2, 2, {8, 1}},
  };
  std::vector<uint64_t> digests;
  Shape shape;
  std::printf("%-28s %6s %9s  items per level\n", "input", "levels", "partials");
  auto report = [&](const char* name) {
    std::printf("%-28s %6d %9lld ", name, shape.levels, (long long)shape.partials);
    for (size_t l = 0; l < shape.items.size(); ++l) std::printf("%s%lld", l ? " / " : " ", (long long)shape.items[l]);
    std::printf("\n");
  };
  for (const Fixed& f : singles) {
    const char* name = f.name;
    digests.push_back(check_case(name, {0, (int32_t)f.len}, 1, 1, &shape));
    report(name);
    if (shape.levels != f.levels || shape.partials != f.partials || shape.items != f.items) FAIL("not the plan sizes written down for this length");
  }
  int hubs3_seen = 0, hubs2_seen = 0;
  for (int64_t R : {1, 3, 33}) {
    for (uint64_t seed = 0; seed < 3; ++seed) {
      const int64_t n_key = R == 33 ? 40 + 30 * (int64_t)seed : (seed == 2 ? 3001 : (R == 1 ? 200 : 70) + 517 * (int64_t)seed);
      const int hubs2 = 2 + (int)seed, hubs3 = seed == 0 ? 0 : (int)seed + 1;     // seed 0: two levels, so a fin_ptr
      const std::string label = "random R=" + std::to_string(R) + " N=" + std::to_string(n_key) + " seed=" + std::to_string(seed);
      const char* name = label.c_str();
      const std::vector<int32_t> rowptr = random_rowptr(seed + 10 * (uint64_t)R, n_key, R, hubs2, hubs3);
      if (rowptr[0] != rowptr[1] || rowptr[rowptr.size() - 1] != rowptr[rowptr.size() - 2]) FAIL("no empty segment at an end");
      digests.push_back(check_case(name, rowptr, n_key, R, &shape));
      report(name);
      if (shape.levels != (hubs3 ? 3 : 2)) FAIL("%d levels with %d three-level hubs", shape.levels, hubs3);
      hubs3_seen += hubs3;
      hubs2_seen += hubs2;
    }
  }
  if (hubs3_seen < 6 || hubs2_seen < 6) return 1;
  if (print_digests) {
    for (uint64_t d : digests) std::printf("    0x%016llXull,\n", (unsigned long long)d);
    return 0;
  }
  const size_t want = sizeof(kParentDigest) / sizeof(kParentDigest[0]);
  if (digests.size() != want) {
    std::printf("plan_check FAILED: %zu fixed inputs, %zu parent digests\n", digests.size(), want);
    return 1;
  }
  for (size_t i = 0; i < want; ++i)
    if (digests[i] != kParentDigest[i]) {
      std::printf("plan_check FAILED: the plan of fixed input #%zu is not the parent's (digest %016llX, parent %016llX)\n", i,
                  (unsigned long long)digests[i], (unsigned long long)kParentDigest[i]);
      return 1;
    }
  if (full) {                                             // the top of the int32 range (too_big() admits E <= 2^31 - 2)
    const int32_t top = 2147483646;
    const auto t0 = std::chrono::steady_clock::now();
    const char* name = "{0, 2147483646}";
    check_case(name, {0, top}, 1, 1, &shape);
    report(name);
    if (shape.levels != 4 || shape.partials != 8388608 + 16384 + 32 || shape.items != std::vector<int64_t>{33554432, 16384, 32, 1})
      FAIL("not the plan sizes of a 2^31 - 2 edge segment");
    name = "{0, 100, 2147483646}";
    check_case(name, {0, 100, top}, 1, 2, &shape);
    report(name);
    if (shape.levels != 4 || shape.partials != 8388608 + 16384 + 32) FAIL("not the plan sizes of a 2^31 - 102 edge segment");
    struct rusage ru;
    getrusage(RUSAGE_SELF, &ru);
    std::printf("top of range: %.1f s, peak resident %ld MB\n",
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), ru.ru_maxrss / 1024);
  }
  std::printf("plan_check ok %zu%s\n", digests.size(), full ? " + top of range" : "");
  return 0;
}
