// The fp32 LDS-DMA k-tile and the streamed walk around it: ONE definition of what k_gemm_nt_dma (rgcn_transform.hip),
// k_rank_count (rank_count.hip), k_topk_select (rank_topk.hip) and k_assign / k_silhouette (cluster.hip) do with a staged
// 64 x (64 TN) x 32 tile - so that an output element is the same k-ordered v_mfma_f32_32x32x2_f32 chain, hence the same
// bits, in all of them - and the loop that streams (column tile, k-tile) pairs through the ring, for those that share it.
//
// Shape: 256 threads as 2 (m) x 2 (n) waves, a wave owns 32 rows x 32 TN columns; k-tile of 32 floats; a ring of
// three LDS buffers [A 64 x 32 | B] filled by `global_load_lds_dwordx4`.  An LDS-DMA wave instruction writes
// 64 x 16 B linearly, so the 128-byte-row tiles (A, and B in B_BLK form) are stored unpadded and bank conflicts are
// removed by XOR-swizzling the 16-byte chunk index with (row >> 1) & 7 - applied to the per-lane SOURCE address on the
// way in (dma_row / dma_col) and to the ds_read_b128 address on the way out (KTile).
// Staging policy - which k-tile goes where, when, from which operand - is walk_tiles below for the kernels with one A
// operand and a range of B_BLK column tiles: k_topk_select, k_assign, k_silhouette.  Two kernels keep a loop of their
// own: k_gemm_nt_dma (two A operands, relation blocks, skipped k-tiles) and k_rank_count (a single column tile per
// workgroup: its loop is the walk's special case, and on the walk it measured 28 % slower - see rank_count.hip).  Both
// have the same shape:
//     wait vmcnt, s_barrier;  tile.read_first(buf_bytes);  <issue the DMAs of k-tile t + 2>;  tile.finish(acc, buf_bytes);
// The ring must be the kernel's first LDS object (LDS address 0): the fragment reads address it absolutely.
#pragma once
#include "rgcn_common.h"

#if defined(__HIPCC__)
namespace mma_f32_dma {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;   // 4 waves, arranged 2 (m) x 2 (n)
constexpr int BK = 32;          // k-tile
constexpr int BM = 64;          // rows of a tile
constexpr int NBUF = 3;         // ring depth

enum { B_KN = 0, B_BLK = 1 };   // LDS form of the B tile: [32 k][BN] as in memory, or [BN][32 k] swizzled like A

__device__ inline void glds16(const float* src, float* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// the swizzle: where 16-byte chunk `chunk` (0..7) of tile row `row` sits inside the row's 128 bytes
__device__ inline int swizzled_chunk(int chunk, int row) { return chunk ^ ((row >> 1) & 7); }

// DMA side of a 128-byte-row tile: wave instruction `inst` fills rows 8 inst .. 8 inst + 7 (LDS destination: the
// tile + inst * 8 * BK floats), eight lanes per row.  The lane's tile row, and the float offset inside the SOURCE row
// it fetches so that its linear 16-byte slot holds the swizzled chunk:
__device__ inline int dma_row(int inst, int lane) { return inst * 8 + (lane >> 3); }
__device__ inline int dma_col(int row, int lane) { return swizzled_chunk(lane & 7, row) << 2; }

template <int TN, int BMODE>
struct KTile {
  static constexpr int NACC = TN;               // accumulators (32 x 32 blocks) of a wave
  static constexpr int BN = 64 * TN;
  static constexpr int A_FLOATS = BM * BK, B_FLOATS = BN * BK, BUF_FLOATS = A_FLOATS + B_FLOATS;
  static constexpr int A_PW = BM / 32;          // A wave-instructions per wave and k-tile (8 rows each)
  static constexpr int B_PW = BN / 32;          // B wave-instructions per wave and k-tile
  static constexpr int P = A_PW + B_PW;         // LDS-DMA instructions per thread and k-tile

  // Fragment reads are inline asm: hipcc cannot tell a ds_read from the in-flight LDS-DMA
  // destinations apart and would drain vmcnt(0) before the first read of every k-tile.
  // Byte addresses inside one buffer, fixed over the k loop (the XOR swizzle is not additive,
  // so the four kb steps get one address register each):
  unsigned a_addr[4], b_addr[TN][4];
  f32x4 fa[2];
  f32x4 fb[2][TN];

  // wave (wm, wn) of the 2 x 2, lane = lh * 32 + li
  __device__ __forceinline__ KTile(int wm, int wn, int li, int lh) {
    const int arow = wm * 32 + li;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      a_addr[s4] = (unsigned)(arow * BK + (swizzled_chunk(2 * s4 + lh, arow) << 2)) * 4u;
#pragma unroll
      for (int b = 0; b < TN; ++b) {
        if (BMODE == B_KN) {
          b_addr[b][s4] = (unsigned)(A_FLOATS + (8 * s4 + 4 * lh) * BN + (wn * TN + b) * 32 + li) * 4u;
        } else {
          const int brow = (wn * TN + b) * 32 + li;
          b_addr[b][s4] = (unsigned)(A_FLOATS + brow * BK + (swizzled_chunk(2 * s4 + lh, brow) << 2)) * 4u;
        }
      }
    }
  }

  static __device__ __forceinline__ unsigned buf_bytes(int buf) { return (unsigned)(buf * BUF_FLOATS) * 4u; }

  __device__ __forceinline__ void read_frags(int set, int s4, unsigned buf_bytes) {
    asm volatile("ds_read_b128 %0, %1" : "=v"(fa[set]) : "v"(a_addr[s4] + buf_bytes));
#pragma unroll
    for (int b = 0; b < TN; ++b) {
      if (BMODE == B_KN) {
        const unsigned ad = b_addr[b][s4] + buf_bytes;
        asm volatile("ds_read_b32 %0, %1" : "=v"(fb[set][b].x) : "v"(ad));
        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(fb[set][b].y) : "v"(ad), "n"(BN * 4));
        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(fb[set][b].z) : "v"(ad), "n"(BN * 8));
        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(fb[set][b].w) : "v"(ad), "n"(BN * 12));
      } else {
        asm volatile("ds_read_b128 %0, %1" : "=v"(fb[set][b]) : "v"(b_addr[b][s4] + buf_bytes));
      }
    }
  }
  // lgkmcnt(0), tied to the registers the MFMAs will read: the compiler sees neither the reads nor the wait as
  // such, and only the register dependence keeps every use (and every copy) of a fragment below its wait
  __device__ __forceinline__ void wait_frags(int set) {
    if (TN == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[set]), "+v"(fb[set][0]), "+v"(fb[set][TN - 1]));
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa[set]), "+v"(fb[set][0]));
  }

  // First piece, right after the barrier that says the buffer has landed: the first fragments of the k-tile go out
  // BEFORE the caller's DMA issue, whose ~40 instructions then cover their LDS latency.
  __device__ __forceinline__ void read_first(unsigned buf_bytes) { read_frags(0, 0, buf_bytes); }

  // Second piece, after the DMA issue: the rest of the k-tile - four steps of eight k each.
  __device__ __forceinline__ void finish(floatx16 (&acc)[TN], unsigned buf_bytes) {
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const int cur = s4 & 1;
      wait_frags(cur);
      if (s4 + 1 < 4) read_frags(cur ^ 1, s4 + 1, buf_bytes);   // in flight behind this step's MFMAs
      __builtin_amdgcn_sched_barrier(0);                        // keep the MFMAs below the reads just issued
#pragma unroll
      for (int b = 0; b < TN; ++b) {
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur].x, fb[cur][b].x, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur].y, fb[cur][b].y, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur].z, fb[cur][b].z, acc[b], 0, 0, 0);
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur].w, fb[cur][b].w, acc[b], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);                        // ... and above the next step's wait
    }
  }
};

// the row inside the wave's 32 that accumulator register r of lane half lh holds (v_mfma_f32_32x32x2_f32)
__device__ __forceinline__ int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// The streamed walk: rows [m0, m0 + 64) of A (clamped to M - 1) against the column tiles [ct_begin, ct_end) of B (row n
// of the product's columns is row brow(n) of B), k-tiles of 32 over d.  The (column tile, k-tile) pairs are ONE stream
// through the ring (`lds`), so the DMA pipeline never drains between column tiles.  pre(ct) runs at the first k-tile of
// a column tile (loads that the epilogue needs go out there, a column tile ahead of their use), epi(ct, acc) after its
// last; the accumulators are zero again behind it.  Tile is a B_BLK KTile.
// One iteration is: wait, barrier, read_first, pre, stage k-tile t + 2, finish (, epi).  The wait is counted, not
// addressed - vmcnt(P): all but the newest P vector-memory operations of this wave are done - and this order is what
// makes the count right.  The loads of pre are issued before the P DMAs of the same iteration, so they sit between two
// groups of P DMAs: at the wait for k-tile t the newest P operations are the DMAs of k-tile t + 1, everything older -
// k-tile t and the loads of pre - has landed, and the loads cost the wait nothing.  What epi issues comes after a
// group of DMAs and only pushes that group further from the newest P: the wait is then stronger than needed, never
// weaker.  (A load issued after the staging would likewise make the next wait hold back DMAs it is meant to leave in
// flight, and a load whose value is used before the epilogue would drain the ring.)
template <class Tile, class BRow, class Pre, class Epi>
__device__ __forceinline__ void walk_tiles(float* lds, const float* __restrict__ A, const float* __restrict__ B, int M,
                                           int d, int m0, int ct_begin, int ct_end, int wave, int lane, Tile& tile,
                                           BRow brow, Pre pre, Epi epi) {
  constexpr int TN = Tile::NACC, BN = Tile::BN, A_FLOATS = Tile::A_FLOATS, BUF_FLOATS = Tile::BUF_FLOATS;
  constexpr int A_PW = Tile::A_PW, B_PW = Tile::B_PW, P = Tile::P;
  floatx16 acc[TN];
#pragma unroll
  for (int b = 0; b < TN; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

  // per-lane source offsets of the LDS-DMAs
  size_t a_off[A_PW];
#pragma unroll
  for (int j = 0; j < A_PW; ++j) {
    const int row = dma_row(wave * A_PW + j, lane);
    const int m = min(m0 + row, M - 1);                        // rows past M read a valid row; never written
    a_off[j] = (size_t)m * d + dma_col(row, lane);
  }
  int b_row[B_PW], b_chunk[B_PW];
  size_t b_off[B_PW];
#pragma unroll
  for (int j = 0; j < B_PW; ++j) {
    b_row[j] = dma_row(wave * B_PW + j, lane);
    b_chunk[j] = dma_col(b_row[j], lane);
    b_off[j] = 0;
  }
  int st_ct = ct_begin, st_kt = 0;                             // next k-tile to stage
  auto stage_next = [&](int buf) {
    if (st_kt == 0) {
#pragma unroll
      for (int j = 0; j < B_PW; ++j) b_off[j] = (size_t)brow(st_ct * BN + b_row[j]) * d + b_chunk[j];
    }
    float* sA = lds + buf * BUF_FLOATS;
    float* sB = sA + A_FLOATS;
#pragma unroll
    for (int j = 0; j < A_PW; ++j) glds16(A + a_off[j] + st_kt, sA + (wave * A_PW + j) * 8 * BK);
#pragma unroll
    for (int j = 0; j < B_PW; ++j) glds16(B + b_off[j] + st_kt, sB + (wave * B_PW + j) * 8 * BK);
    st_kt += BK;
    if (st_kt >= d) { st_kt = 0; ++st_ct; }
  };

  const int KT = d / BK;
  const int total = (ct_end - ct_begin) * KT;                  // k-tiles of the whole walk (>= 1: the host sizes the grid)
  stage_next(0);
  if (total > 1) stage_next(1);

  int cur_ct = ct_begin, cur_kt = 0;                           // k-tile being multiplied
  int buf = 0, buf2 = 2;                                       // ring slots of k-tile t and t + 2
  for (int t = 0; t < total; ++t) {
    // k-tile t landed for this wave (see above; the last k-tile has nothing younger behind it), then for all waves; the
    // barrier also says every wave is done reading the buffer staged next
    if (t + 1 < total) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const unsigned buf_bytes = Tile::buf_bytes(buf);
    tile.read_first(buf_bytes);
    if (cur_kt == 0) pre(cur_ct);
    if (t + 2 < total) stage_next(buf2);
    tile.finish(acc, buf_bytes);
    buf = buf == NBUF - 1 ? 0 : buf + 1;
    buf2 = buf2 == NBUF - 1 ? 0 : buf2 + 1;
    cur_kt += BK;
    if (cur_kt == d) {
      epi(cur_ct, acc);
#pragma unroll
      for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
      cur_kt = 0;
      ++cur_ct;
    }
  }
}

}  // namespace mma_f32_dma
#endif
