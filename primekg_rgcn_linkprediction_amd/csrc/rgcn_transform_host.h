// What the dense transforms decide on the host before a launch, one copy each, as plain host code: the argument rules
// every layer call shares, the row-split plan of the parameter-gradient GEMMs and the layout of their slabs.  No HIP
// include (like rgcn_plan.h), so that the stand-alone host check (tests/transform_host_check.cpp, run under
// AddressSanitizer / UndefinedBehaviorSanitizer) plans exactly what rgcn_transform.hip, rgcn_transform_split.hip and
// rgcn_transform_f16.hip launch.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/rgcn_hip.h"
#include "rgcn_plan.h"

// the shape of a layer call: N nodes, R relations, widths that are multiples of 4 (16-byte rows)
static inline bool rgcn_layer_bad_dims(int64_t n, int64_t r, int64_t di, int64_t dout) {
  return n < 0 || r <= 0 || di <= 0 || dout <= 0 || (di & 3) || (dout & 3);
}

// what the kernels index in 32 bits: rows (twice: a clamped row past the end) and the two widths of the product -
// `k_cols` reduction columns, `n_cols` output columns
static inline bool rgcn_gemm_out_of_range(int64_t rows, int64_t k_cols, int64_t n_cols) {
  return rows > INT32_MAX / 2 || k_cols > (1 << 24) || n_cols > (1 << 24);
}

// one layer of a weight pack (rgcn_weights_split_pack, _pack_multi, rgcn_prep_fill): `need` = the packed bytes of the
// layer; `d_out_multiple`: 4 where several layers are packed at once, 1 (any width) in the single-layer call
static inline int rgcn_pack_layer_check(int64_t R, int64_t d_in, int64_t d_out, int d_out_multiple, const void* weight,
                                        const void* packed, size_t have, size_t need) {
  if (R <= 0 || d_in <= 0 || d_out <= 0 || d_out % d_out_multiple || !weight) return RGCN_ERR_ARG;
  if (rgcn_gemm_out_of_range(0, (R + 1) * d_in, (R + 1) * d_out)) return RGCN_ERR_UNSUPPORTED;
  if (!packed || have < need) return RGCN_ERR_WORKSPACE;
  return RGCN_OK;
}

// ---------------------------------------------------------------------------------------------
// grad_[W ; root][Kc, N] = [agg | x]^T g over M node rows: `kc_tiles` x `n_tiles` output tiles (tkc x 128), each summed
// by `splits` workgroups over `rows_per_split` rows (a multiple of the 32-row m-tile) into a slab of its own; the
// fixed-order sum of the slabs is k_slab_reduce.  As many splits as `target_blocks` workgroups allow, none under 128 rows.
// ---------------------------------------------------------------------------------------------
struct rgcn_tn_split { int kc_tiles, n_tiles, splits, rows_per_split; };

static inline rgcn_tn_split rgcn_tn_plan(int64_t M, int64_t Kc, int64_t N, int tkc, int target_blocks) {
  rgcn_tn_split p;
  p.kc_tiles = (int)ceil_div64(Kc, tkc);
  p.n_tiles = (int)ceil_div64(N, 128);
  const int tiles = p.kc_tiles * p.n_tiles;
  int64_t s = std::max<int64_t>(1, target_blocks / tiles);
  s = std::min<int64_t>(s, std::max<int64_t>(1, ceil_div64(M, 128)));
  int64_t rps = ceil_div64(ceil_div64(M, s), 32) * 32;
  if (rps < 32) rps = 32;
  p.rows_per_split = (int)rps;
  p.splits = (int)std::max<int64_t>(1, ceil_div64(M, rps));
  return p;
}

// Workgroups per launch of the fp32 kernels.  Slab bytes (and the reduce that follows) scale with the count, so a
// graph of C2's size gets one workgroup per CU (measured best); once every workgroup still has
// >= 2,048 rows to stream, two per CU are worth their slabs: the second wave per SIMD covers
// the per-tile barrier (C4 on one GPU: 2.5 -> 2.0 ms per launch).
static inline int rgcn_tn_target_blocks(int64_t M, int tiles) {
  return M / std::max(1, 512 / tiles) >= 2048 ? 512 : 256;
}

// The workspace of such a launch: `splits` slabs of [kc_rows, N] floats, then `splits` rows of column sums of g (the
// grad_bias partials).  kc_rows is (R + 1) * d_in whether or not a root gradient is wanted: the size does not depend on it.
struct rgcn_slab_layout {
  size_t slab_floats, bias_floats;
  size_t bytes() const { return (slab_floats + bias_floats) * sizeof(float); }
};
static inline rgcn_slab_layout rgcn_slab_layout_of(const rgcn_tn_split& p, int64_t kc_rows, int64_t N) {
  return {(size_t)p.splits * kc_rows * N, (size_t)p.splits * N};
}

// the reduction a launch into that layout leaves pending: K1 rows of grad_weight, Kc - K1 of grad_root
static inline void rgcn_slab_job_fill(rgcn_slab_job* job, void* workspace, const rgcn_slab_layout& l, int splits, int K1,
                                      int Kc, int64_t N, float* grad_weight, float* grad_root, float* grad_bias) {
  const float* slab = (const float*)workspace;
  *job = rgcn_slab_job{slab, slab + l.slab_floats, splits, K1, Kc, (int32_t)N, grad_weight, grad_root, grad_bias};
}

// What both parameter-gradient "begin" calls ask before they plan: an empty job first (a refused call leaves nothing
// pending), then shape, operands, `k_multiple` (the split kernel's 64-column kc half-tile lies in one relation; 0: no
// such rule) and the index range.
static inline int rgcn_params_begin_check(rgcn_slab_job* job, const float* agg, const float* x, const float* g, int64_t N,
                                          int64_t R, int64_t d_in, int64_t d_out, const float* grad_weight,
                                          int k_multiple) {
  if (!job) return RGCN_ERR_ARG;
  *job = rgcn_slab_job{};
  if (rgcn_layer_bad_dims(N, R, d_in, d_out) || !grad_weight) return RGCN_ERR_ARG;
  if (N > 0 && (!agg || !x || !g)) return RGCN_ERR_ARG;
  if (k_multiple && d_in % k_multiple) return RGCN_ERR_UNSUPPORTED;
  if (rgcn_gemm_out_of_range(N, (R + 1) * d_in, d_out)) return RGCN_ERR_UNSUPPORTED;
  return RGCN_OK;
}
