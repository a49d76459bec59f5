// Stand-alone host check of csrc/rgcn_transform_host.h (built and run by tests/test_transform_host.py under
// AddressSanitizer / UndefinedBehaviorSanitizer): rgcn_tn_plan against a verbatim copy of the two planners it replaced -
// the fp32 file's plan_splits (64-column kc tiles, one or two workgroups per CU) and the split-precision file's tn_plan
// (128-column kc tiles, 256 workgroups) - over N x R x d_in x d_out, field by field, plus what the kernels rely on:
// whole 32-row m-tiles per split, every row in exactly one split, no empty split, and the section sizes of the slab
// workspace.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "primekg_rgcn_linkprediction_amd/csrc/rgcn_transform_host.h"

namespace before {   // the planners as they stood in rgcn_transform.hip and rgcn_transform_split.hip

struct SplitPlan { int kc_tiles, n_tiles, splits, rows_per_split; };

int tn_target_blocks(int64_t M, int tiles) {
  return M / std::max(1, 512 / tiles) >= 2048 ? 512 : 256;
}

SplitPlan plan_splits(int64_t M, int64_t Kc, int64_t N) {
  SplitPlan p;
  p.kc_tiles = (int)ceil_div64(Kc, 64);
  p.n_tiles = (int)ceil_div64(N, 128);
  const int tiles = p.kc_tiles * p.n_tiles;
  int64_t s = std::max<int64_t>(1, tn_target_blocks(M, tiles) / tiles);
  s = std::min<int64_t>(s, std::max<int64_t>(1, ceil_div64(M, 128)));
  int64_t rps = ceil_div64(ceil_div64(M, s), 32) * 32;
  if (rps < 32) rps = 32;
  p.rows_per_split = (int)rps;
  p.splits = (int)std::max<int64_t>(1, ceil_div64(M, rps));
  return p;
}

struct TnPlan { int kc_tiles, n_tiles, splits, rows_per_split; };

TnPlan tn_plan(int64_t M, int64_t Kc, int64_t N) {
  TnPlan p;
  p.kc_tiles = (int)ceil_div64(Kc, 128);
  p.n_tiles = (int)ceil_div64(N, 128);
  const int tiles = p.kc_tiles * p.n_tiles;
  const int target = 256;
  int64_t s = std::max<int64_t>(1, target / tiles);
  s = std::min<int64_t>(s, std::max<int64_t>(1, ceil_div64(M, 128)));
  int64_t rps = ceil_div64(ceil_div64(M, s), 32) * 32;
  if (rps < 32) rps = 32;
  p.rows_per_split = (int)rps;
  p.splits = (int)std::max<int64_t>(1, ceil_div64(M, rps));
  return p;
}

}  // namespace before

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (++failures <= 20) {            \
        printf("FAIL %s: ", #cond);      \
        printf(__VA_ARGS__);             \
        printf("\n");                    \
      }                                  \
    }                                    \
  } while (0)

template <class P>
static bool same(const rgcn_tn_split& a, const P& b) {
  return a.kc_tiles == b.kc_tiles && a.n_tiles == b.n_tiles && a.splits == b.splits && a.rows_per_split == b.rows_per_split;
}

static void invariants(const rgcn_tn_split& p, int64_t M, int64_t Kc, int64_t N, int tkc, int target) {
  CHECK(p.rows_per_split >= 32 && p.rows_per_split % 32 == 0, "M=%lld rps=%d", (long long)M, p.rows_per_split);
  CHECK(p.splits >= 1 && (int64_t)p.splits * p.rows_per_split >= M, "M=%lld splits=%d rps=%d", (long long)M, p.splits, p.rows_per_split);
  if (M > 0) CHECK((int64_t)(p.splits - 1) * p.rows_per_split < M, "an empty split: M=%lld splits=%d rps=%d", (long long)M, p.splits, p.rows_per_split);
  CHECK((int64_t)p.kc_tiles * tkc >= Kc && (int64_t)(p.kc_tiles - 1) * tkc < Kc, "Kc=%lld kc_tiles=%d", (long long)Kc, p.kc_tiles);
  CHECK((int64_t)p.n_tiles * 128 >= N && (int64_t)(p.n_tiles - 1) * 128 < N, "N=%lld n_tiles=%d", (long long)N, p.n_tiles);
  // no more workgroups than asked for, unless the tiles alone are more
  CHECK((int64_t)p.splits * p.kc_tiles * p.n_tiles <= std::max(target, p.kc_tiles * p.n_tiles), "M=%lld Kc=%lld N=%lld", (long long)M, (long long)Kc, (long long)N);
  const rgcn_slab_layout lay = rgcn_slab_layout_of(p, Kc, N);
  CHECK(lay.slab_floats == (size_t)p.splits * (size_t)Kc * (size_t)N, "slab section");
  CHECK(lay.bias_floats == (size_t)p.splits * (size_t)N, "bias section");
  CHECK(lay.bytes() == ((size_t)p.splits * Kc * N + (size_t)p.splits * N) * sizeof(float), "bytes");
  float base[4];
  rgcn_slab_job job{};
  float gw, gr, gb;
  rgcn_slab_job_fill(&job, base, lay, p.splits, (int)(Kc - 4), (int)Kc, N, &gw, &gr, &gb);
  CHECK(job.slab == base && (size_t)(job.bias_part - job.slab) == lay.slab_floats && job.splits == p.splits &&
            job.K1 == Kc - 4 && job.Kc == Kc && job.N == N && job.grad_weight == &gw && job.grad_root == &gr && job.grad_bias == &gb,
        "job");
}

int main() {
  const int64_t Ns[] = {0, 1, 31, 32, 33, 127, 128, 129, 4096, 30926, 262144, 4200000};
  const int64_t Rs[] = {1, 3, 33};
  const int64_t ds[] = {4, 32, 64, 96, 128, 256};
  int shapes = 0, one_split = 0, many = 0, two_per_cu = 0;
  for (int64_t M : Ns)
    for (int64_t R : Rs)
      for (int64_t d_in : ds)
        for (int64_t d_out : ds) {
          const int64_t Kc = (R + 1) * d_in;
          const int tiles = (int)(ceil_div64(Kc, 64) * ceil_div64(d_out, 128));
          const int target = rgcn_tn_target_blocks(M, tiles);
          CHECK(target == before::tn_target_blocks(M, tiles), "M=%lld tiles=%d", (long long)M, tiles);
          const rgcn_tn_split a = rgcn_tn_plan(M, Kc, d_out, 64, target), b = rgcn_tn_plan(M, Kc, d_out, 128, 256);
          CHECK(same(a, before::plan_splits(M, Kc, d_out)), "fp32 plan: M=%lld Kc=%lld N=%lld", (long long)M, (long long)Kc, (long long)d_out);
          CHECK(same(b, before::tn_plan(M, Kc, d_out)), "split plan: M=%lld Kc=%lld N=%lld", (long long)M, (long long)Kc, (long long)d_out);
          invariants(a, M, Kc, d_out, 64, target);
          invariants(b, M, Kc, d_out, 128, 256);
          ++shapes;
          one_split += a.splits == 1;
          many += a.splits > 1;
          two_per_cu += target == 512;
        }
  CHECK(one_split > 0 && many > 0 && two_per_cu > 0 && two_per_cu < shapes, "the grid must see both sides: %d %d %d", one_split, many, two_per_cu);

  // the argument rules
  CHECK(!rgcn_layer_bad_dims(0, 1, 4, 4) && rgcn_layer_bad_dims(-1, 1, 4, 4) && rgcn_layer_bad_dims(1, 0, 4, 4) &&
            rgcn_layer_bad_dims(1, 1, 6, 4) && rgcn_layer_bad_dims(1, 1, 4, 6) && rgcn_layer_bad_dims(1, 1, 0, 4), "dims");
  CHECK(!rgcn_gemm_out_of_range(INT32_MAX / 2, 1 << 24, 1 << 24) && rgcn_gemm_out_of_range(INT32_MAX / 2 + 1, 4, 4) &&
            rgcn_gemm_out_of_range(1, (1 << 24) + 1, 4) && rgcn_gemm_out_of_range(1, 4, (1 << 24) + 1), "range");
  const int w = 0;
  CHECK(rgcn_pack_layer_check(3, 64, 64, 4, &w, &w, 100, 100) == RGCN_OK, "pack");
  CHECK(rgcn_pack_layer_check(3, 64, 62, 4, &w, &w, 100, 100) == RGCN_ERR_ARG && rgcn_pack_layer_check(3, 64, 62, 1, &w, &w, 100, 100) == RGCN_OK, "pack width");
  CHECK(rgcn_pack_layer_check(3, 64, 64, 4, nullptr, nullptr, 0, 100) == RGCN_ERR_ARG, "pack: arguments first");
  CHECK(rgcn_pack_layer_check(3, 1 << 23, 64, 4, &w, nullptr, 0, 100) == RGCN_ERR_UNSUPPORTED, "pack: then the range");
  CHECK(rgcn_pack_layer_check(3, 64, 64, 4, &w, nullptr, 100, 100) == RGCN_ERR_WORKSPACE && rgcn_pack_layer_check(3, 64, 64, 4, &w, &w, 99, 100) == RGCN_ERR_WORKSPACE, "pack: then the buffer");
  rgcn_slab_job job{};
  job.splits = 7;
  const float f = 0.f;
  CHECK(rgcn_params_begin_check(nullptr, &f, &f, &f, 1, 1, 64, 64, &f, 0) == RGCN_ERR_ARG, "begin: no job");
  CHECK(rgcn_params_begin_check(&job, &f, &f, &f, 1, 1, 62, 64, &f, 0) == RGCN_ERR_ARG && job.splits == 0, "begin: empties the job");
  CHECK(rgcn_params_begin_check(&job, nullptr, &f, &f, 0, 1, 64, 64, &f, 64) == RGCN_OK, "begin: N == 0 needs no operands");
  CHECK(rgcn_params_begin_check(&job, nullptr, &f, &f, 1, 1, 32, 64, &f, 64) == RGCN_ERR_ARG, "begin: operands before the k rule");
  CHECK(rgcn_params_begin_check(&job, &f, &f, &f, 1, 1, 32, 64, &f, 64) == RGCN_ERR_UNSUPPORTED && rgcn_params_begin_check(&job, &f, &f, &f, 1, 1, 32, 64, &f, 0) == RGCN_OK, "begin: k rule");

  if (failures) {
    printf("transform_host_check FAILED: %d\n", failures);
    return 1;
  }
  printf("transform_host_check ok %d shapes\n", shapes);
  return 0;
}
