// Candidate filters of the masked ranking pass (distmult_rank_masked: k_rank_count in rank_count.hip) and of the
// top-k pass (rank_topk.hip) as bit masks over the entities: bit (n & 31) of word (n >> 5), W = ceil(N / 32)
// words per row - the layout in which one ballot word of the ranking epilogue meets exactly one mask word.
//   exclude[b] : the known positives of query b (filtered ranking, Bordes et al.), from a CSR of known triples
//   allow[c]   : the entities of class c (type-constrained ranking), from a node-class vector
// Nothing here knows about ranks: a top-k epilogue over the same scores can take the same masks.
#include "rgcn_common.h"

namespace {

constexpr int kThreads = 256;

// One workgroup per query: it clears its own row and sets its own bits, so the launch needs no memset before it
// and no two workgroups touch the same word.  An id outside [0, N) (or a segment outside the CSR) raises the
// library's index-error flag and writes nothing.
__global__ __launch_bounds__(kThreads) void k_exclude_bits(const int64_t* __restrict__ ptr, const int64_t* __restrict__ ids,
                                                           const int64_t* __restrict__ seg, int64_t num_segments,
                                                           int64_t nnz, int N, int words, uint32_t* __restrict__ out,
                                                           int* __restrict__ index_error) {
  uint32_t* row = out + (size_t)blockIdx.x * words;
  for (int w = threadIdx.x; w < words; w += kThreads) row[w] = 0u;
  const int64_t s = seg[blockIdx.x];
  if (s < 0) return;                                   // nothing known for this query (uniform over the workgroup)
  if (s >= num_segments) {
    if (threadIdx.x == 0) *index_error = 1;
    return;
  }
  const int64_t lo = ptr[s], hi = ptr[s + 1];
  if (lo < 0 || hi < lo || hi > nnz) {
    if (threadIdx.x == 0) *index_error = 1;
    return;
  }
  // the zeros above are plain stores, the bits below are atomics executed at the L2: every thread's zeros must have
  // arrived there before any thread's first atomic
  __threadfence();
  __syncthreads();
  for (int64_t e = lo + threadIdx.x; e < hi; e += kThreads) {
    const int64_t id = ids[e];
    if ((uint64_t)id >= (uint64_t)N) *index_error = 1;
    else atomicOr(&row[id >> 5], 1u << (id & 31));
  }
}

// One wave per 64 entities = two words of every class row; every word of allow is written (zeros included).
__global__ __launch_bounds__(kThreads) void k_allow_bits(const int32_t* __restrict__ class_of, int N, int num_classes,
                                                         int words, uint32_t* __restrict__ allow,
                                                         int* __restrict__ index_error) {
  const int n = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63;
  const int w0 = (n - lane) >> 5;                      // first of the wave's two words
  int c = n < N ? class_of[n] : -1;                    // negative: in no class
  if (c >= num_classes) {
    *index_error = 1;
    c = -1;
  }
  for (int k = 0; k < num_classes; ++k) {
    const unsigned long long in = __ballot(c == k);
    if (lane < 2 && w0 + lane < words)
      allow[(size_t)k * words + w0 + lane] = lane ? (uint32_t)(in >> 32) : (uint32_t)in;
  }
}

}  // namespace

extern "C" {

int rgcn_rank_exclude_bits(const int64_t* ptr, const int64_t* ids, const int64_t* seg, int64_t num_segments, int64_t nnz,
                           int64_t batch, int64_t num_entities, uint32_t* exclude, void* stream_) {
  if (batch < 0 || num_entities <= 0 || num_segments < 0 || nnz < 0) return RGCN_ERR_ARG;
  if (batch == 0) return RGCN_OK;
  if (!seg || !exclude || (num_segments > 0 && (!ptr || (nnz > 0 && !ids)))) return RGCN_ERR_ARG;
  if (batch > INT32_MAX / 2 || num_entities > INT32_MAX / 2) return RGCN_ERR_UNSUPPORTED;
  RGCN_ALIGN_TRY(8, ptr, ids, seg);
  RGCN_ALIGN_TRY(4, exclude);
  hipStream_t stream = (hipStream_t)stream_;
  int* flag = rgcn_index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  k_exclude_bits<<<(unsigned)batch, kThreads, 0, stream>>>(ptr, ids, seg, num_segments, nnz, (int)num_entities,
                                                          (int)ceil_div64(num_entities, 32), exclude, flag);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

int rgcn_rank_allow_bits(const int32_t* class_of, int64_t num_entities, int64_t num_classes, uint32_t* allow,
                         void* stream_) {
  if (num_entities <= 0 || num_classes <= 0 || !class_of || !allow) return RGCN_ERR_ARG;
  const int64_t words = ceil_div64(num_entities, 32);
  if (num_entities > INT32_MAX / 2 || num_classes * words > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  RGCN_ALIGN_TRY(4, class_of, allow);
  hipStream_t stream = (hipStream_t)stream_;
  int* flag = rgcn_index_error_flag();
  if (!flag) return RGCN_ERR_HIP;
  k_allow_bits<<<(unsigned)ceil_div64(num_entities, kThreads), kThreads, 0, stream>>>(class_of, (int)num_entities,
                                                                                     (int)num_classes, (int)words, allow, flag);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // extern "C"
