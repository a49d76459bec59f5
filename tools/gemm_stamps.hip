// Where the time of one transform launch goes: the split-precision NT / TN kernels compiled with RGCN_STAMPS (thread 0
// of every workgroup writes the 100 MHz wall clock at entry, main loop reached, main loop left, end), driven with C2's
// shapes on synthetic data.  Prints, per kernel: the launch's device time (events), and over the workgroups the spread
// of the entry times (dispatch ramp), the three phase lengths (prologue / main loop / epilogue) and the exit times, then
// the placement: how many workgroups each CU received and how far apart in blockIdx the workgroups of one CU are.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -DRGCN_STAMPS tools/gemm_stamps.hip -o tools/gemm_stamps && tools/gemm_stamps
#include "../primekg_rgcn_linkprediction_amd/csrc/rgcn_transform_split.hip"

#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

__global__ void k_fill(float* p, size_t n, unsigned seed) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u + seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    p[i] = ((float)(h & 0xffff) / 32768.f - 1.f) * 0.05f;
  }
}

static void report(const char* name, int wgs, float ms) {
  std::vector<unsigned long long> st(8192 * 4);
  hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(g_rgcn_stamps), st.size() * sizeof(unsigned long long));
  wgs = std::min(wgs, 8192);
  unsigned long long t0 = ~0ull, t3 = 0;
  for (int w = 0; w < wgs; ++w) { t0 = std::min(t0, st[w * 4]); t3 = std::max(t3, st[w * 4 + 3]); }
  auto stats = [&](auto f, const char* what) {
    std::vector<double> v(wgs);
    for (int w = 0; w < wgs; ++w) v[w] = f(w) * 0.01;           // 100 MHz ticks -> us
    std::sort(v.begin(), v.end());
    printf("    %-28s min %6.2f  median %6.2f  p90 %6.2f  max %6.2f us\n", what, v[0], v[wgs / 2], v[wgs * 9 / 10], v[wgs - 1]);
  };
  printf("%s: %d workgroups, launch %.2f us (events), first entry -> last exit %.2f us\n", name, wgs, ms * 1e3, (t3 - t0) * 0.01);
  stats([&](int w) { return (double)(st[w * 4] - t0); }, "entry after first entry");
  stats([&](int w) { return (double)(st[w * 4 + 1] - st[w * 4]); }, "prologue");
  stats([&](int w) { return (double)(st[w * 4 + 2] - st[w * 4 + 1]); }, "main loop");
  stats([&](int w) { return (double)(st[w * 4 + 3] - st[w * 4 + 2]); }, "epilogue");
  stats([&](int w) { return (double)(st[w * 4 + 3] - st[w * 4]); }, "workgroup lifetime");
  stats([&](int w) { return (double)(t3 - st[w * 4 + 3]); }, "exit before last exit");
  // which workgroups share a CU: key = XCC id and the SE / SH / CU fields of HW_ID (bits 15:8)
  std::vector<unsigned> hw(8192);
  hipMemcpyFromSymbol(hw.data(), HIP_SYMBOL(g_rgcn_stamp_cu), hw.size() * sizeof(unsigned));
  std::map<unsigned, std::vector<int>> cus;
  std::map<unsigned, int> xcd_of_mod8;
  bool mod8 = true;
  for (int w = 0; w < wgs; ++w) {
    cus[hw[w] & 0xffffff00u].push_back(w);
    auto it = xcd_of_mod8.emplace((unsigned)(w % 8), (int)(hw[w] >> 16)).first;
    mod8 = mod8 && it->second == (int)(hw[w] >> 16);
  }
  std::map<int, int> per_cu, gap;
  for (auto& c : cus) {
    ++per_cu[(int)c.second.size()];
    for (size_t i = 1; i < c.second.size(); ++i) ++gap[c.second[i] - c.second[i - 1]];
  }
  printf("    placement: %zu CUs used, blockIdx %% 8 %s the XCD;", cus.size(), mod8 ? "fixes" : "does NOT fix");
  for (auto& p : per_cu) printf("  %d CUs with %d workgroup%s", p.second, p.first, p.first == 1 ? "" : "s");
  printf("\n    blockIdx distance between workgroups of one CU (distance: pairs):");
  std::vector<std::pair<int, int>> g(gap.begin(), gap.end());
  std::sort(g.begin(), g.end(), [](auto& a, auto& b) { return a.second > b.second; });
  for (size_t i = 0; i < g.size() && i < 8; ++i) printf("  %d: %d", g[i].first, g[i].second);
  printf("\n    main loop of the workgroups that share a CU / have one alone (median us):");
  std::vector<double> shared, alone;
  for (auto& c : cus)
    for (int w : c.second) (c.second.size() > 1 ? shared : alone).push_back((st[w * 4 + 2] - st[w * 4 + 1]) * 0.01);
  std::sort(shared.begin(), shared.end()); std::sort(alone.begin(), alone.end());
  printf("  %.2f (%zu) / %.2f (%zu)\n", shared.empty() ? 0. : shared[shared.size() / 2], shared.size(),
         alone.empty() ? 0. : alone[alone.size() / 2], alone.size());
}

int main(int argc, char** argv) {
  const int64_t N = 30926, R = 3, d_out = 128;
  hipStream_t stream;
  CHECK(hipStreamCreate(&stream));
  hipEvent_t beg, end;
  CHECK(hipEventCreate(&beg));
  CHECK(hipEventCreate(&end));
  for (int64_t d_in : {64, 128}) {
    const int64_t K1 = R * d_in;
    float *agg, *x, *g, *w, *root, *bias, *out, *gw, *groot, *gbias, *amax;
    CHECK(hipMalloc(&agg, N * K1 * 4)); CHECK(hipMalloc(&x, N * d_in * 4)); CHECK(hipMalloc(&g, N * d_out * 4));
    CHECK(hipMalloc(&w, K1 * d_out * 4)); CHECK(hipMalloc(&root, d_in * d_out * 4)); CHECK(hipMalloc(&bias, d_out * 4));
    CHECK(hipMalloc(&out, N * d_out * 4)); CHECK(hipMalloc(&gw, K1 * d_out * 4)); CHECK(hipMalloc(&groot, d_in * d_out * 4));
    CHECK(hipMalloc(&gbias, d_out * 4)); CHECK(hipMalloc(&amax, 4 * RGCN_AMAX_FLOATS * 4));
    k_fill<<<1024, 256, 0, stream>>>(agg, N * K1, 1); k_fill<<<1024, 256, 0, stream>>>(x, N * d_in, 2);
    k_fill<<<1024, 256, 0, stream>>>(g, N * d_out, 3); k_fill<<<64, 256, 0, stream>>>(w, K1 * d_out, 4);
    k_fill<<<64, 256, 0, stream>>>(root, d_in * d_out, 5); k_fill<<<1, 128, 0, stream>>>(bias, d_out, 6);
    const size_t pbytes = rgcn_weights_split_bytes(R, d_in, d_out);
    void* packed; CHECK(hipMalloc(&packed, pbytes));
    const size_t nt_ws = rgcn_transform_split_workspace_bytes(R, d_in, d_out), tn_ws = rgcn_transform_bwd_params_split_workspace_bytes(N, R, d_in, d_out);
    void *ws1, *ws2; CHECK(hipMalloc(&ws1, nt_ws)); CHECK(hipMalloc(&ws2, tn_ws));
    float *ax = amax, *ag = amax + RGCN_AMAX_FLOATS, *aa = amax + 2 * RGCN_AMAX_FLOATS;
    rgcn_absmax(x, N * d_in, ax, nullptr, 0, stream); rgcn_absmax(g, N * d_out, ag, nullptr, 0, stream);
    rgcn_absmax(agg, N * K1, aa, nullptr, 0, stream);
    rgcn_weights_split_pack(w, root, R, d_in, d_out, packed, pbytes, stream);
    auto timed = [&](auto launch, const char* name, int wgs) {
      for (int i = 0; i < 5; ++i) launch();
      hipEventRecord(beg, stream);
      for (int i = 0; i < 20; ++i) launch();
      hipEventRecord(end, stream);
      hipStreamSynchronize(stream);
      float ms = 0.f;
      hipEventElapsedTime(&ms, beg, end);
      launch();                                                  // the launch whose stamps are read
      hipStreamSynchronize(stream);
      report(name, wgs, ms / 20.f);
    };
    char name[128];
    snprintf(name, sizeof name, "NT forward  [%lld x %lld] x [%lld x %lld]", (long long)N, (long long)(K1 + d_in), (long long)(K1 + d_in), (long long)d_out);
    const int half = getenv("RGCN_STAMP_HALF") ? 1 : 0;           // one-pass fp16 arithmetic (configs[4]'s GEMMs)
    timed([&] { rgcn_transform_fwd_split(agg, x, w, root, packed, bias, 1, nullptr, N, R, d_in, d_out, aa, 1.f, ax, half, out, nullptr, ws1,
                                         nt_ws, stream, nullptr, 0, nullptr); }, name, (int)((N + 63) / 64));
    // the same launch under each relation mask given on the command line (one uint32 word per 32-row tile, as
    // `tools/row_order_probe.py masks DIR` writes them for each row labelling of C2's graph)
    for (int a = 1; a < argc; ++a) {
      const size_t words = (size_t)((N + 31) / 32);
      std::vector<uint32_t> host(words);
      FILE* fh = fopen(argv[a], "rb");
      if (!fh || fread(host.data(), 4, words, fh) != words) { printf("cannot read %zu mask words from %s\n", words, argv[a]); return 1; }
      fclose(fh);
      uint32_t* tmask; CHECK(hipMalloc(&tmask, words * 4));
      CHECK(hipMemcpy(tmask, host.data(), words * 4, hipMemcpyHostToDevice));
      snprintf(name, sizeof name, "NT forward, K = %lld, relation mask %s", (long long)(K1 + d_in), argv[a]);
      timed([&] { rgcn_transform_fwd_split(agg, x, w, root, packed, bias, 1, tmask, N, R, d_in, d_out, aa, 1.f, ax, half, out, nullptr, ws1,
                                           nt_ws, stream, nullptr, 0, nullptr); }, name, (int)((N + 63) / 64));
      CHECK(hipFree(tmask));
    }
    rgcn_slab_job job;
    snprintf(name, sizeof name, "TN params   [%lld x %lld]^T x [%lld x %lld]", (long long)N, (long long)(K1 + d_in), (long long)N, (long long)d_out);
    const rgcn_tn_split p = rgcn_tn_plan(N, K1 + d_in, d_out, TN_TKC, kTnBlocks);
    timed([&] { rgcn_transform_bwd_params_split_begin(agg, x, g, nullptr, N, R, d_in, d_out, aa, 1.f, ax, ag, 0, gw, groot, gbias, ws2,
                                                      tn_ws, stream, &job); }, name, p.kc_tiles * p.n_tiles * p.splits);
    hipFree(agg); hipFree(x); hipFree(g); hipFree(w); hipFree(root); hipFree(bias); hipFree(out); hipFree(gw); hipFree(groot);
    hipFree(gbias); hipFree(amax); hipFree(packed); hipFree(ws1); hipFree(ws2);
  }
  return 0;
}
