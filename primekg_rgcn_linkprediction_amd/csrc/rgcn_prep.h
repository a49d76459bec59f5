// The first launch of a pass - max |x| of its input table, cleared amax buffers, the layers' split weight images -
// as device bodies templated on the workgroup size (k_absmax_multi, k_pack_split, k_absmax_pack of
// rgcn_transform_split.hip).  Round 3 also ran them as 256-thread riders at the front of
// conv1's gather (rgcn_aggregate_prep, in git history): bit-identical and 5 us per step SLOWER - each rider scans its
// layer's weights for their maximum itself, 8 rounds of loads in 256 threads instead of 2 in 1,024, and outlasts the
// gather it was meant to hide behind (profiles/r03_prep_rides.txt).  Same values whatever the workgroup size (a
// maximum has no order; every element is split by itself).
#pragma once
#include "rgcn_split.h"

constexpr int RGCN_PACK_JOBS = 4, RGCN_PREP_TENSORS = 8;
constexpr int RGCN_PREP_ZERO_MAX = 1024;         // amax buffers one launch clears on the side (the accepted zero_count)
#ifndef RGCN_STAMP
#define RGCN_STAMP(i)                             // (tools/pack_probe.hip builds with the stamps of rgcn_transform_split.hip)
#endif

struct rgcn_pack_job {
  const float *W, *Rt;
  int R, d_in, d_out;
  const float *w_amax, *r_amax;                  // amax buffers of W and root (rgcn_absmax_multi), or NULL: scan here
  __half *Bh_f, *Bl_f, *Bh_b, *Bl_b;
  __half *Fh_f, *Fl_f, *Fh_b, *Fl_b;             // the same two images in MFMA B-fragment order (see k_pack_split)
  __half *Bh_n, *Bl_n;                           // [W ; root] in its own order [(r, i)][o]: the transform-first image
  float* scale_out;
  int tiled, nblocks;                            // (rgcn_pack_plan) body and workgroups of this layer
};
struct rgcn_pack_jobs {
  rgcn_pack_job j[RGCN_PACK_JOBS];
};

// Widths that are multiples of 32 are packed by 32 (i) x 32 (o) tiles of one block r of [W ; root], one tile per team
// of 256 threads or more: every image receives whole aligned runs from such a tile (64-byte rows of the three row-major
// images, two whole 1 KB blocks of each fragment image), so the tile is read ONCE, as float4, and every image is
// written with 16-byte stores - an eighth of the store instructions of the element-wise body, which runs on a store
// tail bound by their number.  Other widths keep the element-wise body.
constexpr int RGCN_PACK_TILE = 32, RGCN_PACK_TEAM = 256;
constexpr int RGCN_PACK_PITCH = 40;              // halves per LDS row of a tile: 16-byte aligned rows, 8 halves of padding
constexpr int RGCN_PACK_TEAM_LDS = 4 * RGCN_PACK_TILE * RGCN_PACK_PITCH * 2;   // [hi | lo][i-major | o-major] of a tile
template <int TILES>
constexpr int rgcn_pack_lds_bytes() {            // up to 16 floats of the reduction, then the teams' tiles
  return 64 + TILES * RGCN_PACK_TEAM_LDS;
}

// the body and the workgroups of one layer: `tiles` tiles (tiled) or `threads` elements to a workgroup and trip, at
// most `cap` workgroups
inline void rgcn_pack_plan(rgcn_pack_job* j, int threads, int tiles, int cap) {
  const int64_t blocks = j->R + (j->Rt ? 1 : 0);
  j->tiled = !(j->d_in % RGCN_PACK_TILE) && !(j->d_out % RGCN_PACK_TILE);
  const int64_t units = j->tiled ? blocks * (j->d_in / RGCN_PACK_TILE) * (j->d_out / RGCN_PACK_TILE) : blocks * j->d_in * j->d_out;
  const int64_t per = j->tiled ? tiles : threads;
  const int64_t n = (units + per - 1) / per;
  j->nblocks = (int)(n < cap ? n : cap);
}

// max |[W ; root]| of the job: from the amax buffers the pass's first launch left, or scanned here (SCAN = false: a
// launch whose jobs all bring their maxima is compiled without the scan and its registers)
template <int THREADS, bool SCAN>
__device__ inline float rgcn_pack_amax(const rgcn_pack_job& J, float* red) {
  const float* __restrict__ W = J.W;
  const float* __restrict__ Rt = J.Rt;
  const int lane = threadIdx.x & 63;
  float m = 0.f;
  if (!SCAN || J.w_amax) {                       // maxima left by the pass's first launch: four loads per lane
    m = rgcn_amax_value(J.w_amax, lane);
    if (Rt) m = fmaxf(m, rgcn_amax_value(J.r_amax, lane));
  } else {
    const int64_t wn4 = (int64_t)J.R * J.d_in * J.d_out / 4, rn4 = Rt ? (int64_t)J.d_in * J.d_out / 4 : 0;   // d_out % 4 == 0
    // W and root as ONE index range, 16,384 float4 per round whatever the workgroup size: [W ; root] of a 128 x 128
    // layer is a single round of independent loads (the scan is the head of this workgroup's latency chain: every
    // round is a memory round trip).  Every load is UNCONDITIONAL, from an index clamped into the range (an element
    // read twice leaves the maximum alone): a load under `i < n ? p[i] : 0` is compiled as a branch with a full
    // s_waitcnt vmcnt(0) where it joins, and the "round" was sixteen round trips in a row (profiles/first_launch.txt).
    constexpr int U = SCAN ? 16384 / THREADS : 1;
    const float4* __restrict__ w4 = reinterpret_cast<const float4*>(W);
    const float4* __restrict__ r4 = reinterpret_cast<const float4*>(Rt);
    const int64_t n4 = wn4 + rn4;
    for (int64_t i0 = threadIdx.x; i0 < n4; i0 += U * THREADS) {
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = min(i0 + (int64_t)u * THREADS, n4 - 1);
        const float4* __restrict__ at = i < wn4 ? w4 + i : r4 + (i - wn4);
        v[u] = *at;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v[u].x), fabsf(v[u].y))), fmaxf(fabsf(v[u].z), fabsf(v[u].w)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = red[lane & (THREADS / 64 - 1)];
#pragma unroll
    for (int o = THREADS / 128; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  }
  return m;
}

// The tiled body.  A workgroup is TILES teams of THREADS / TILES >= 256 threads; team `team` of workgroup `bid` takes
// tiles (bid + k nblocks) * TILES + team, k = 0, 1, ...  The first 256 threads of a team load and split its tile - the
// first tile's load is issued ahead of the maximum's loads (scanned or given), one round trip for both - and the
// whole team stores it: 1,024 items (4 readings of the tile x hi | lo x 128 chunks of 16 bytes), a wave on one reading.
template <int THREADS, bool SCAN, int TILES>
__device__ inline void rgcn_pack_tiles(const rgcn_pack_job& J, unsigned char* lds, int bid) {
  constexpr int TS = THREADS / TILES, T = RGCN_PACK_TILE, P = RGCN_PACK_PITCH;
  static_assert(TS >= RGCN_PACK_TEAM && TS * TILES == THREADS && 1024 % TS == 0, "a team loads its tile with 256 threads");
  const int R = J.R, d_in = J.d_in, d_out = J.d_out, nblocks = J.nblocks;
  const int blocks = R + (J.Rt ? 1 : 0);
  const int NTb = d_in / T, NTf = d_out / T, tiles = blocks * NTb * NTf;
  const int Kf = blocks * d_in, Kb = blocks * d_out;
  const int team = threadIdx.x / TS, t = threadIdx.x % TS;
  const bool loader = t < RGCN_PACK_TEAM;
  const int il = (t >> 3) & (T - 1), o4 = (t & 7) * 4;   // the float4 a loader loads: row il, columns o4 .. o4 + 3 of the tile
  // (unconditional, for every thread and from a clamped tile: a load under a condition would be waited for where its
  // branch joins, ahead of the maximum's loads - rgcn_pack_amax)
  auto load = [&](int tile_) -> float4 {         // tile = (r * NTb + it) * NTf + ot
    const int tile = min(tile_, tiles - 1);
    const int ot = tile % NTf, it = (tile / NTf) % NTb, r = tile / (NTf * NTb);
    const float* base = r < R ? J.W + (size_t)r * d_in * d_out : J.Rt;
    return *reinterpret_cast<const float4*>(base + (size_t)(it * T + il) * d_out + ot * T + o4);
  };
  int group = bid;                               // TILES tiles; uniform over the workgroup
  int tile = group * TILES + team;
  float4 raw = load(tile);
  const float m = rgcn_pack_amax<THREADS, SCAN>(J, reinterpret_cast<float*>(lds));
  const int eb = scale_exponent(m);
  const float sb = pow2f(eb);
  RGCN_STAMP(1);                                  // the maximum is known
  if (bid == 0 && threadIdx.x == 0) J.scale_out[0] = pow2f(-eb);
  // the team's tile in LDS, hi then lo, each i-major ([i][o]) then o-major ([o][i]), rows of P halves
  unsigned short* tl = reinterpret_cast<unsigned short*>(lds + 64 + team * RGCN_PACK_TEAM_LDS);
  // hi or lo image by lane, as arithmetic on the two (uniform) pointers: `hl ? lo : hi` on fields of the job is compiled
  // as a per-lane LOAD of the chosen field, a memory round trip ahead of every store
  auto pick = [](__half* hi, __half* lo, int hl) -> __half* {
    return hi + hl * (lo - hi);                  // (both lie in one packed buffer)
  };
  __half* const Bh_b = J.Bh_b; __half* const Bl_b = J.Bl_b; __half* const Bh_n = J.Bh_n; __half* const Bl_n = J.Bl_n;
  __half* const Bh_f = J.Bh_f; __half* const Bl_f = J.Bl_f; __half* const Fh_b = J.Fh_b; __half* const Fl_b = J.Fl_b;
  __half* const Fh_f = J.Fh_f; __half* const Fl_f = J.Fl_f;
  for (;;) {
    if (loader && tile < tiles) {
      const float x[4] = {raw.x, raw.y, raw.z, raw.w};
      unsigned short h[4], l[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = x[q] * sb;
        const __half hi = __float2half_rn(v);
        h[q] = __half_as_ushort(hi);
        l[q] = __half_as_ushort(__float2half_rn(v - __half2float(hi)));
      }
      *reinterpret_cast<uint2*>(tl + il * P + o4) = make_uint2(h[0] | (unsigned)h[1] << 16, h[2] | (unsigned)h[3] << 16);
      *reinterpret_cast<uint2*>(tl + 2 * T * P + il * P + o4) = make_uint2(l[0] | (unsigned)l[1] << 16, l[2] | (unsigned)l[3] << 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        tl[T * P + (o4 + q) * P + il] = h[q];
        tl[3 * T * P + (o4 + q) * P + il] = l[q];
      }
    }
    __syncthreads();
    if (tile < tiles) {
      const int ot = tile % NTf, it = (tile / NTf) % NTb, r = tile / (NTf * NTb);
      const int i0 = it * T, o0 = ot * T;
#pragma unroll
      for (int w = t; w < 1024; w += TS) {
        const int reading = w >> 8, hl = (w >> 7) & 1, c = w & 127;
        const unsigned short* Ai = tl + (2 * hl) * T * P;
        const unsigned short* Ao = Ai + T * P;
        // rows: chunk c is 8 consecutive k of row c / 4 (64-byte runs, four lanes each)
        const int row = c >> 2, col = (c & 3) * 8;
        // fragments: chunk c is lane c & 63 of the tile's block c >> 6 - n = c & 31, k = 8 (c >> 5) .. + 7 of the
        // tile; each wave writes 1 KB in one piece
        const int n = c & 31, k = 8 * (c >> 5);
        if (reading == 0) {                                                          // i = row, o = col .. col + 7
          const uint4 v = *reinterpret_cast<const uint4*>(Ai + row * P + col);
          *reinterpret_cast<uint4*>(pick(Bh_b, Bl_b, hl) + (size_t)(i0 + row) * Kb + (size_t)r * d_out + o0 + col) = v;
          *reinterpret_cast<uint4*>(pick(Bh_n, Bl_n, hl) + ((size_t)r * d_in + i0 + row) * d_out + o0 + col) = v;
        } else if (reading == 1) {                                                   // o = row, i = col .. col + 7
          const uint4 v = *reinterpret_cast<const uint4*>(Ao + row * P + col);
          *reinterpret_cast<uint4*>(pick(Bh_f, Bl_f, hl) + (size_t)(o0 + row) * Kf + (size_t)r * d_in + i0 + col) = v;
        } else if (reading == 2) {                                                   // n = i, k = o
          const uint4 v = *reinterpret_cast<const uint4*>(Ai + n * P + k);
          const size_t s0 = (size_t)(r * d_out + o0) / 16 + (c >> 6);
          *reinterpret_cast<uint4*>(pick(Fh_b, Fl_b, hl) + ((s0 * NTb + it) * 64 + (c & 63)) * 8) = v;
        } else {                                                                     // n = o, k = i
          const uint4 v = *reinterpret_cast<const uint4*>(Ao + n * P + k);
          const size_t s0 = (size_t)(r * d_in + i0) / 16 + (c >> 6);
          *reinterpret_cast<uint4*>(pick(Fh_f, Fl_f, hl) + ((s0 * NTf + ot) * 64 + (c & 63)) * 8) = v;
        }
      }
    }
    group += nblocks;
    if (group * TILES >= tiles) break;
    tile = group * TILES + team;
    raw = load(tile);
    __syncthreads();                             // the tile in LDS has been read by everyone
  }
  RGCN_STAMP(2);                                  // every store issued
}

// workgroup bid of the job (THREADS threads each, J.nblocks of them work); lds: rgcn_pack_lds_bytes<TILES>(), 16-aligned
template <int THREADS, bool SCAN, int TILES>
__device__ inline void rgcn_pack_body(const rgcn_pack_job& J, unsigned char* lds, int bid) {
  const int nblocks = J.nblocks;
  if (bid >= nblocks) return;                    // (a launch is as wide as its widest layer)
  if (J.tiled) return rgcn_pack_tiles<THREADS, SCAN, TILES>(J, lds, bid);
  const float* __restrict__ W = J.W;
  const float* __restrict__ Rt = J.Rt;
  const int R = J.R, d_in = J.d_in, d_out = J.d_out;
  const float m = rgcn_pack_amax<THREADS, SCAN>(J, reinterpret_cast<float*>(lds));
  const int eb = scale_exponent(m);
  const float sb = pow2f(eb);
  RGCN_STAMP(1);                                  // the maximum is known
  if (bid == 0 && threadIdx.x == 0) J.scale_out[0] = pow2f(-eb);
  __half* __restrict__ Bh_f = J.Bh_f;
  __half* __restrict__ Bl_f = J.Bl_f;
  __half* __restrict__ Bh_b = J.Bh_b;
  __half* __restrict__ Bl_b = J.Bl_b;
  const int blocks = R + (Rt ? 1 : 0);
  const int Kf = blocks * d_in, Kb = blocks * d_out;
  const int64_t total = (int64_t)blocks * d_in * d_out;
  // Element e of EACH image in one trip: the stores of every image are contiguous over e (2-byte stores a whole row
  // apart cost this launch twice its time), the strided side is a 4-byte read of L2-resident weights - and the
  // reads of a trip are issued together (separate passes per image made this a chain of round trips).
  // Fragment order (widths that are multiples of 32 only: rgcn_pack_tiles): element ((s * NT + nt) * 64 + lane) * 8 + j is
  // image[n = 32 nt + (lane & 31)][k = 16 s + 8 (lane >> 5) + j] - a wave's B operand of one
  // v_mfma_f32_32x32x16_f16 is ONE coalesced 16-byte-per-lane read, no LDS staging (the fused layer kernels keep
  // these fragments in registers).
  auto source = [&](int r, int i, int o) -> const float* {
    return r < R ? W + ((size_t)r * d_in + i) * d_out + o : Rt + (size_t)i * d_out + o;
  };
  auto split = [&](float raw, __half* __restrict__ hi, __half* __restrict__ lo, size_t at) {
    const float v = raw * sb;
    const __half h = __float2half_rn(v);
    hi[at] = h;
    lo[at] = __float2half_rn(v - __half2float(h));
  };
  for (int64_t e = (int64_t)bid * THREADS + threadIdx.x; e < total; e += (int64_t)nblocks * THREADS) {
    // backward image, o fastest (its k): element e is (r, i, o) of [W ; root] itself
    const int ob = (int)(e % d_out), ib = (int)((e / d_out) % d_in), rb = (int)(e / ((int64_t)d_out * d_in));
    // forward image, i fastest (its k)
    const int i_f = (int)(e % d_in), r_f = (int)((e / d_in) % blocks), o_f = (int)(e / ((int64_t)d_in * blocks));
    const float vb = *source(rb, ib, ob), vf = *source(r_f, i_f, o_f);
    split(vb, Bh_b, Bl_b, (size_t)ib * Kb + (size_t)rb * d_out + ob);
    split(vb, J.Bh_n, J.Bl_n, (size_t)e);        // natural order: n = r * d_in + i, k = o (T = g * [W_r^T | root^T])
    split(vf, Bh_f, Bl_f, (size_t)o_f * Kf + (size_t)r_f * d_in + i_f);
  }
  RGCN_STAMP(2);                                  // every store issued
}

struct rgcn_absmax_multi_job {
  const float* p[RGCN_PREP_TENSORS];
  int64_t n[RGCN_PREP_TENSORS];
  float* out[RGCN_PREP_TENSORS];
  int count;
};

// Head `bid` of nblocks = RGCN_AMAX_HEADS receives the maximum over float4 i with (i / 1024) % nblocks == bid, whatever
// THREADS: a workgroup takes its 1,024-float4 pieces in slices of THREADS, four pieces to a round of loads.
// CLAMPED: the loads of a round are unconditional, from a clamped index (k_absmax_pack); otherwise each is read under
// its bound, which the compiler turns into a branch and a wait per load - measured no slower for the maxima-only
// launch, and faster where most of its tensors are small (profiles/first_launch.txt), so that launch keeps it.
template <int THREADS, bool CLAMPED>
__device__ inline void rgcn_absmax_body(const rgcn_absmax_multi_job& J, float* __restrict__ zero, int zero_count, float* red,
                                   int bid, int nblocks) {      // workgroup bid of nblocks = RGCN_AMAX_HEADS
  constexpr int PIECE = 1024, S = PIECE / THREADS;
  for (int t = 0; t < J.count; ++t) {
    const float* __restrict__ p = J.p[t];
    const int64_t n = J.n[t], n4 = n >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(p);
    float m = 0.f;
    const int64_t stride = (int64_t)nblocks * PIECE;
    for (int64_t i0 = (int64_t)bid * PIECE + threadIdx.x; i0 < n4; i0 += 4 * stride) {
      // 4 S loads per thread and round; what lies past the end counts as 0, so that a head holds the maximum of its
      // own pieces only
      float4 v[4 * S];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const int64_t i = i0 + u * stride + s * THREADS;
          if (CLAMPED) v[u * S + s] = p4[min(i, n4 - 1)];
          else v[u * S + s] = i < n4 ? p4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const float4 q = v[u * S + s];
          const float mu = fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fmaxf(fabsf(q.z), fabsf(q.w)));
          m = fmaxf(m, i0 + u * stride + s * THREADS < n4 ? mu : 0.f);
        }
    }
    if (bid == 0 && threadIdx.x < (n & 3)) m = fmaxf(m, fabsf(p[n4 * 4 + threadIdx.x]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      float mm = red[0];
#pragma unroll
      for (int w = 1; w < THREADS / 64; ++w) mm = fmaxf(mm, red[w]);
      J.out[t][bid * RGCN_AMAX_HEAD_STRIDE] = mm;
    }
    __syncthreads();
  }
  for (int z = (int)threadIdx.x; z < zero_count; z += THREADS)
    zero[(size_t)z * RGCN_AMAX_FLOATS + bid * RGCN_AMAX_HEAD_STRIDE] = 0.f;
}

// one rider: the arguments of k_absmax_pack, for workgroups of `threads` threads
struct rgcn_prep {
  rgcn_absmax_multi_job J;
  float* zero;
  int zero_count;
  rgcn_pack_jobs JJ;
  int pack_blocks, layers;       // pack_blocks workgroups per layer, then RGCN_AMAX_HEADS for the scan
};
// validates the arguments of rgcn_absmax_pack and fills the rider for workgroups of `threads` threads
// (rgcn_transform_split.hip; RGCN_OK or an error code)
__attribute__((visibility("hidden"))) int rgcn_prep_fill(const float* x, int64_t numel, float* x_amax, float* zero_buffers,
                                                         int zero_count, int count, const float* const* weights,
                                                         const float* const* roots, const int64_t* R, const int64_t* d_in,
                                                         const int64_t* d_out, void* const* packed,
                                                         const size_t* packed_bytes, int threads, rgcn_prep* out);
