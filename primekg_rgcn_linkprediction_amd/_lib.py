"""ctypes binding of ``librgcn_hip.so`` (C ABI declared in ``include/rgcn_hip.h``).

There is no CPU fallback: if the library is missing, or was built against another
ABI version, every compute entry point raises.  ``import torch`` must precede the
``dlopen`` so that the HIP runtime already in the process (torch's bundled
``libamdhip64.so.7``) satisfies the library's NEEDED entry by soname.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_double, c_float, POINTER, c_char_p, c_int, c_int64, c_size_t, c_void_p

import torch  # noqa: F401  (loads the HIP runtime first)

ABI_VERSION = 38
LIB_NAME = "librgcn_hip.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

RGCN_OK = 0
RGCN_ERR_ARG = -1
RGCN_ERR_RANGE = -2
RGCN_ERR_HIP = -3
RGCN_ERR_UNSUPPORTED = -4
RGCN_ERR_WORKSPACE = -5
RGCN_ERR_ALIGN = -6

_P = c_void_p      # device pointers travel as integers (tensor.data_ptr())
_I64 = c_int64

class SlabJob(ctypes.Structure):
    """``rgcn_slab_job``: a pending parameter-gradient slab reduction (plain device pointers)."""
    _fields_ = [("slab", c_void_p), ("bias_part", c_void_p), ("splits", ctypes.c_int32), ("K1", ctypes.c_int32),
                ("Kc", ctypes.c_int32), ("N", ctypes.c_int32), ("grad_weight", c_void_p), ("grad_root", c_void_p),
                ("grad_bias", c_void_p)]


class SeqArg(ctypes.Structure):
    """``rgcn_seq_arg``"""
    _fields_ = [("kind", ctypes.c_int32), ("index", ctypes.c_int32), ("value", ctypes.c_int64)]


class SeqCall(ctypes.Structure):
    """``rgcn_seq_call``"""
    _fields_ = [("fn", ctypes.c_int32), ("num_args", ctypes.c_int32), ("first_arg", ctypes.c_int64)]


SEQ_IMM, SEQ_FLOAT, SEQ_BASE, SEQ_JOB, SEQ_STREAM, SEQ_ARRAY = range(6)
SEQ_MAX_JOBS = 8    # RGCN_SEQ_MAX_JOBS
# entry points rgcn_sequence_run can forward to, in the header's RGCN_FN_* order: name -> position of `void* stream`
SEQ_FUNCTIONS = {
    "rgcn_absmax": 5, "rgcn_absmax_multi": 6, "rgcn_absmax_pack": 13, "rgcn_weights_split_pack_multi": 12,
    "rgcn_aggregate": 7, "rgcn_aggregate_ex": 12,
    "rgcn_transform_fwd_split": 20, "rgcn_transform_bwd_input_split": 19, "rgcn_transform_first_split": 12,
    "rgcn_transform_bwd_params_split_begin": 18, "rgcn_slab_reduce": 1, "rgcn_layer_fwd_fused": 17,
    "rgcn_layer_bwd_input_fused": 17, "rgcn_transform_bwd_input_chain_split": 18,
}
# their HOST array parameters: position -> (entries are device pointers?, position of the parameter holding the count)
SEQ_HOST_ARRAYS = {
    "rgcn_absmax_multi": {1: (True, 0), 2: (False, 0), 3: (True, 0)},
    "rgcn_absmax_pack": {6: (True, 5), 7: (True, 5), 8: (False, 5), 9: (False, 5), 10: (False, 5), 11: (True, 5), 12: (False, 5)},
    "rgcn_weights_split_pack_multi": {1: (True, 0), 2: (True, 0), 3: (False, 0), 4: (False, 0), 5: (False, 0), 6: (True, 0),
                                      7: (True, 0), 8: (True, 0), 9: (False, 0)},
}


# The C boundary: one table per header of include/, name -> (restype, argtypes), each mirroring its header one to one;
# HEADERS below is the registry that load() and the tests enumerate.  rgcn_hip.h is the training path: error codes, ABI
# version, graph handles, and the only entry points rgcn_sequence_run may forward (SEQ_FUNCTIONS above).  Every other
# header includes it for those conventions, declares entry points rgcn_hip.h does not know, and is never forwarded:
# its calls (sampling, analysis, baselines, other heads, queries) happen outside any recorded Region.
PROTOTYPES = {
    "rgcn_abi_version": (c_int, []),
    "rgcn_strerror": (c_char_p, [c_int]),
    "rgcn_graph_create": (c_int, [_P, _P, _I64, _I64, _I64, _P, POINTER(c_void_p)]),
    "rgcn_graph_create_bipartite": (c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, POINTER(c_void_p)]),
    "rgcn_graph_destroy": (None, [c_void_p]),
    "rgcn_graph_num_edges": (_I64, [c_void_p]),
    "rgcn_graph_num_nodes": (_I64, [c_void_p]),
    "rgcn_graph_num_relations": (_I64, [c_void_p]),
    "rgcn_graph_num_levels": (c_int, [c_void_p, c_int]),
    "rgcn_graph_weight_bound": (c_float, [c_void_p, c_int]),
    "rgcn_graph_arrays": (c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_void_p),
                                  POINTER(c_void_p), POINTER(c_void_p)]),
    "rgcn_graph_export": (c_int, [c_void_p, c_int, _P, _P, _P, _P, _P]),
    "rgcn_graph_import": (c_int, [_I64, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P, POINTER(c_void_p)]),
    "rgcn_aggregate_workspace_bytes": (c_size_t, [c_void_p, c_int, _I64]),
    "rgcn_aggregate": (c_int, [c_void_p, c_int, _P, _I64, _P, _P, c_size_t, _P]),
    "rgcn_aggregate_ex": (c_int, [c_void_p, c_int, _P, c_int, _I64, _P, _P, c_size_t, c_int, c_int, POINTER(SlabJob), _P, _P]),
    "rgcn_graph_tile_mask": (c_void_p, [c_void_p, c_int, POINTER(c_int64)]),
    "rgcn_transform_fwd": (c_int, [_P, _P, _P, _P, _P, c_int, _P, _I64, _I64, _I64, _I64, _P, _P]),
    "rgcn_transform_fwd_f16_workspace_bytes": (c_size_t, [_I64, _I64, _I64]),
    "rgcn_transform_fwd_f16": (c_int, [_P, _P, _P, _P, _P, c_int, _P, _I64, _I64, _I64, _I64, _P, _P, c_size_t, _P]),
    "rgcn_transform_bwd_input": (c_int, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _P]),
    "rgcn_transform_bwd_params_workspace_bytes": (c_size_t, [_I64, _I64, _I64, _I64]),
    "rgcn_transform_bwd_params": (c_int, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, _P, _P,
                                          c_size_t, _P]),
    "rgcn_transform_bwd_params_begin": (c_int, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, _P, _P, _P, c_size_t, _P,
                                                POINTER(SlabJob)]),
    "rgcn_slab_reduce": (c_int, [POINTER(SlabJob), _P]),
    "rgcn_absmax": (c_int, [_P, _I64, _P, _P, c_int, _P]),
    "rgcn_absmax_multi": (c_int, [c_int, _P, _P, _P, _P, c_int, _P]),
    "rgcn_absmax_pack": (c_int, [_P, _I64, _P, _P, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "rgcn_weights_split_pack_multi": (c_int, [c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P]),
    "rgcn_weights_split_bytes": (c_size_t, [_I64, _I64, _I64]),
    "rgcn_weights_split_pack": (c_int, [_P, _P, _I64, _I64, _I64, _P, c_size_t, _P]),
    "rgcn_transform_split_workspace_bytes": (c_size_t, [_I64, _I64, _I64]),
    "rgcn_transform_fwd_split": (c_int, [_P, _P, _P, _P, _P, _P, c_int, _P, _I64, _I64, _I64, _I64, _P, c_float, _P, c_int,
                                         _P, _P, _P, c_size_t, _P, c_void_p, c_int, _P]),
    "rgcn_transform_bwd_input_split": (c_int, [_P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, c_float, _P, c_int,
                                               _P, _P, _P, c_size_t, _P, c_void_p, c_int, _P, c_float]),
    "rgcn_transform_bwd_input_chain_supported": (c_int, [_I64, _I64, _I64, _I64, _I64]),
    "rgcn_transform_bwd_input_chain_split": (c_int, [_P, _P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, c_float, _P, _P,
                                                     _P, _P, c_size_t, _P, c_void_p, c_int, _P, c_float, _P, c_int, _I64,
                                                     _I64, _P]),
    "rgcn_aggregate_deferrable": (c_int, [c_void_p, c_int, _I64]),
    "rgcn_transform_first_split": (c_int, [_P, _P, c_int, _I64, _I64, _I64, _I64, _P, c_int, _P, _P, c_size_t, _P]),
    "rgcn_transform_bwd_params_split_workspace_bytes": (c_size_t, [_I64, _I64, _I64, _I64]),
    "rgcn_transform_bwd_params_split_begin": (c_int, [_P, _P, _P, _P, _I64, _I64, _I64, _I64, _P, c_float, _P, _P, c_int,
                                                      _P, _P, _P, _P, c_size_t, _P, POINTER(SlabJob)]),
    "rgcn_layer_fwd_fused_supported": (c_int, [_I64, _I64, _I64]),
    "rgcn_layer_fwd_fused": (c_int, [_P, _P, _P, _I64, _I64, _P, _P, _P, c_int, _P, c_int, _I64, _I64, _P, _P, _P, _P, _P]),
    "rgcn_layer_bwd_input_fused_supported": (c_int, [_I64, _I64, _I64]),
    "rgcn_layer_bwd_input_fused": (c_int, [_P, _P, _P, _P, _I64, _I64, _P, _P, _P, c_int, _P, _I64, _I64, _P, c_float, _P, _P,
                                           _P, c_float, _P]),
    "rgcn_sequence_run": (c_int, [_P, c_int, _P, _I64, _P, c_int, _P]),
    "distmult_fwd": (c_int, [_P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _I64, _I64, _P, _P]),
    "rgcn_index_error_fetch": (c_int, [POINTER(c_int), _P]),
    "distmult_bwd_workspace_bytes": (c_size_t, [_I64, _I64, _I64]),
    "rgcn_segment_sum_workspace_bytes": (c_size_t, [_I64, _I64, _I64]),
    "rgcn_segment_sum": (c_int, [_P, _P, _I64, _I64, _I64, _P, _P, c_size_t, _P]),
    "distmult_rank_tails": (c_int, [_P, _P, _P, _P, _I64, _I64, _I64, _P, _P]),
    "distmult_rank_masked": (c_int, [_P, _P, _P, _P, _P, _P, _I64, _P, _I64, _I64, _I64, _P, _P]),
    "rgcn_rank_exclude_bits": (c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _P, _P]),
    "rgcn_rank_allow_bits": (c_int, [_P, _I64, _I64, _P, _P]),
    "distmult_topk_workspace_bytes": (c_size_t, [_I64, _I64, _I64, _I64]),
    "distmult_topk_masked": (c_int, [_P, _P, _P, _P, _I64, _P, c_float, _I64, _I64, _I64, _I64, _I64, _P, _P, _P,
                                     c_size_t, _P]),
    "rgcn_basis_compose": (c_int, [_P, _P, _I64, _I64, _I64, _P, _P]),
    "rgcn_basis_compose_bwd_workspace_bytes": (c_size_t, [_I64, _I64, _I64]),
    "rgcn_basis_compose_bwd": (c_int, [_P, _P, _P, _I64, _I64, _I64, _P, _P, _P, c_size_t, _P]),
    "distmult_bce_reduce": (c_int, [_P, _P, _P, _I64, _P, _P, _P, _P, _I64, _P]),
    "distmult_score_all_tails": (c_int, [_P, _P, _P, _I64, _P, _I64, _I64, _I64, _P, _P, _P]),
    "distmult_bwd": (c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _I64, _I64, _P, _P, _P, _P, c_size_t, c_int, _P]),
    "rgcn_adam_workspace_bytes": (c_size_t, [c_int, _P]),
    "rgcn_adam_clip_step": (c_int, [c_int, _P, _P, _P, _P, _P, _P, c_float, c_double, c_double, c_float, c_float, c_int,
                                    c_float, _P, _P, _P, c_size_t, _P]),
    "rgcn_sample_batch": (c_int, [_P, _P, _I64, _P, _P, _I64, _I64, _I64, _P, _P, _P, _P, _P, _P]),
    "distmult_bce_fwd": (c_int, [_P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _P, _I64, _I64, _P, _P, _P]),
    "distmult_bce_bwd": (c_int, [_P, _P, _P, _P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _I64, _I64, _P, _P, _P, _P,
                                 c_size_t, c_int, _P]),
}

# rgcn_sampling.h: the protocol-aware batch sampler (csrc/sampler_constrained.hip)
SAMPLING_PROTOTYPES = {
    "rgcn_sample_batch_constrained": (c_int, [_P, _P, _I64, _P, _P, _I64, _I64, _I64, _P,          # slice, cursor, rng
                                              _P, _P, _P, _I64,                                    # classes
                                              _P, _P, _P, _I64, _I64, _P, _P, _P, _I64, _I64, _I64,   # known triples
                                              c_int, _P,                                           # max_tries, stats
                                              _P, _P, _P, _P, _P]),
}

# rgcn_paths.h: score-ranked connecting paths between node pairs (csrc/paths.hip)
PATHS_PROTOTYPES = {
    "rgcn_edge_cosine": (c_int, [_P, _I64, c_int, _P, _P, _I64, _P, _P]),
    "rgcn_paths_workspace_bytes": (c_size_t, [_I64, c_int, c_int]),
    "rgcn_paths_topk": (c_int, [_P, _P, _P, _P, _P, _P, _I64, _I64,            # structure, edge scores
                                _P, _P, _I64, c_int, c_int, c_int,             # queries, max_len, k, slices
                                _P, _P, _P, _P, _P, c_size_t, _P]),            # outputs, workspace, stream
}

# rgcn_cluster.h: k-means and silhouette analysis of embedding rows (csrc/cluster.hip)
CLUSTER_PROTOTYPES = {
    "rgcn_kmeans_workspace_bytes": (c_size_t, [_I64, _I64, _I64, _I64]),
    "rgcn_kmeans_assign": (c_int, [_P, _I64, _I64, _P, _I64, _I64,                # rows, centroids
                                   _P, _P, _P, _P, _P, c_size_t, _P]),            # labels, counters, flags, workspace, stream
    "rgcn_kmeans_update": (c_int, [_P, _I64, _I64, _P, _I64, _I64,
                                   _P, _P, _P, _P, _P, _P, c_float, _P, c_size_t, _P]),
    "rgcn_kmeans_inertia": (c_int, [_P, _I64, _I64, _P, _I64, _I64, _P, _P, _P, c_size_t, _P]),
    "rgcn_silhouette_workspace_bytes": (c_size_t, [_I64, _I64, _I64, _I64]),
    "rgcn_silhouette_samples": (c_int, [_P, _P, _P, _P, _P, _P, _I64, _I64, _I64, _I64, _I64, _P, _P, _P, c_size_t, _P]),
}

# rgcn_tsne.h: t-SNE projection of embedding rows to the plane (csrc/tsne.hip)
TSNE_PROTOTYPES = {
    "rgcn_knn_refine": (c_int, [_P, _I64, _I64, _P, _I64, _P, _P, _P]),
    "rgcn_tsne_affinities": (c_int, [_P, _I64, _I64, c_double, _P, _P, _P]),
    "rgcn_tsne_workspace_bytes": (c_size_t, [_I64, _I64]),
    "rgcn_tsne_gradient": (c_int, [_P, _I64, _P, _P, _P, _I64, c_float, _I64, c_int,       # layout, P, options
                                   _P, _P, _P, _P, c_size_t, _P]),                         # outputs, workspace, stream
    "rgcn_tsne_update": (c_int, [_P, _I64, c_float, c_float, c_float, _P, _P, _P, _P, _P, c_size_t, _P]),
}

# rgcn_neighborhood.h: local-neighbourhood statistics of node pairs (csrc/neighborhood.hip)
NEIGHBORHOOD_PROTOTYPES = {
    "rgcn_neighborhood_max_nodes": (_I64, []),
    "rgcn_pair_neighborhood": (c_int, [_P, _P, _P, _P, _I64, _I64,                 # structure
                                       _P, _P, _I64, c_int,                        # queries, radius
                                       _P, c_int, c_int,                           # node classes, common_cap
                                       _P, _P, _P, _P, _P, _P, _P, _P]),           # outputs, stream
}

# rgcn_transe.h: one batch-synchronous TransE training step (csrc/transe.hip)
TRANSE_PROTOTYPES = {
    "rgcn_transe_step_workspace_bytes": (c_size_t, [_I64, _I64, _I64]),
    "rgcn_transe_step": (c_int, [_P, _I64, _P, _I64, _I64,                         # tables
                                 _P, _P, _P, _I64, c_float, c_float,               # batch, lr, margin
                                 _P, _P, _P, _P, c_size_t, _P]),                   # loss outputs, workspace, stream
}

# rgcn_resample.h: bootstrap resampling of the evaluation metrics (csrc/resample.hip)
RESAMPLE_PROTOTYPES = {
    "rgcn_resample_weights": (c_int, [_I64, _I64, _I64, _P, _P]),
    "rgcn_resample_curves": (c_int, [_P, _P, _P, _I64, _I64, _I64, _I64, _I64,     # sorted samples, cut, units, replicates, seed
                                     _P, _P, _P, _P, _P, _P, _P]),                 # wp, wn, auc2, ap, tp, fp, stream
    "rgcn_resample_ranks": (c_int, [_P, _P, _I64, _P, c_int, _I64, _I64, _I64,     # ranks, k_values, units, replicates, seed
                                    _P, _P, _P, _P, _P]),                          # w_sum, rank_sum, hits, rr_sum, stream
}
RESAMPLE_TILE = 1024             # RGCN_RESAMPLE_TILE
RESAMPLE_MAX_SAMPLES = 1 << 28   # RGCN_RESAMPLE_MAX_SAMPLES
RESAMPLE_MAX_REPLICATES = 65535  # RGCN_RESAMPLE_MAX_REPLICATES
RESAMPLE_MAX_K = 8               # RGCN_RESAMPLE_MAX_K

# rgcn_complex.h: the ComplEx scoring head (csrc/complex.hip); parameter for parameter the DistMult head's rows
COMPLEX_PROTOTYPES = {
    "complex_fwd": (c_int, [_P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _I64, _I64, _P, _P]),
    "complex_bce_fwd": (c_int, [_P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _P, _I64, _I64, _P, _P, _P]),
    "complex_bwd_workspace_bytes": (c_size_t, [_I64, _I64, _I64]),
    "complex_bwd": (c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _I64, _I64, _P, _P, _P, _P, c_size_t, c_int, _P]),
    "complex_bce_bwd": (c_int, [_P, _P, _P, _P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _I64, _I64, _P, _P, _P, _P,
                                c_size_t, c_int, _P]),
    "rgcn_complex_query": (c_int, [c_int, _P, _P, _I64, _P, _P, _I64, _I64, _I64, _P, _P]),
}

# rgcn_softmax.h: the 1-vs-all softmax loss over every candidate (csrc/softmax_loss.hip)
SOFTMAX_PROTOTYPES = {
    "rgcn_softmax_workspace_bytes": (c_size_t, [_I64, _I64, _I64, _I64]),
    "rgcn_softmax_lse": (c_int, [_P, _P, _P, _P, _P, _I64, _P, _I64, _I64, _I64, _I64,     # operands, masks, sizes, slices
                                 _P, _P, _P, _P, _P, _P, c_size_t, _P]),                   # outputs, workspace, stream
    "rgcn_softmax_grad": (c_int, [_P, _P, _P, _P, _P, _P, _I64, _P, _P, _I64, _I64, _I64, _I64,
                                  _P, _P, c_int, _P, c_size_t, _P]),                       # dq, dE, accumulate, workspace, stream
}
SOFTMAX_MAX_D = 256              # widest row the backward keeps in accumulators (csrc/softmax_loss.hip)

# rgcn_edge_dropout.h: edge dropout and hidden batch edges, drawn before the forward (csrc/edge_dropout.hip)
EDGE_DROPOUT_PROTOTYPES = {
    "rgcn_edge_dropout_create": (c_int, [c_void_p, _P, POINTER(c_void_p)]),
    "rgcn_edge_dropout_destroy": (None, [c_void_p]),
    "rgcn_edge_dropout_graph": (c_void_p, [c_void_p]),
    "rgcn_edge_dropout_kept": (c_void_p, [c_void_p]),
    "rgcn_edge_dropout_kept_export": (c_int, [c_void_p, _P, _P]),
    "rgcn_edge_dropout_draw": (c_int, [c_void_p, c_double, _P, _P, _I64, _P, _P, _P]),   # p, rng, cursor, batch, position, stats
}
EDGE_DROPOUT_STREAM = 0x45444F50   # RGCN_EDGE_DROPOUT_STREAM
EDGE_DROPOUT_HIDE_TWINS, EDGE_DROPOUT_PAIRED = 1 << 62, 1 << 61   # option bits of the draw's `batch`
EDGE_DROPOUT_MASK = 1 << 60        # RGCN_EDGE_DROPOUT_MASK: the mask draw - `rng` is float mask[E], nothing is drawn
EDGE_DROPOUT_ATTENTION = 1 << 59   # RGCN_EDGE_DROPOUT_ATTENTION: the attention draw - `rng` is float a[2 * N * R], p the slope

# rgcn_sparse.h: the row-granular occupancy behind sparse aggregates (csrc/rgcn_graph.hip).  MODE_SPARSE_ROWS:
# RGCN_MODE_SPARSE_ROWS of rgcn_hip.h, the bit a training pass sets in the `int` option word of its gathers and of the
# split transforms that read their aggregates.
SPARSE_PROTOTYPES = {
    "rgcn_graph_row_mask": (c_void_p, [c_void_p, c_int, POINTER(c_int64)]),
    "rgcn_occupancy_host": (_I64, [_P, _I64, _I64, _P, POINTER(c_int64)]),
}
MODE_SPARSE_ROWS = 2


# rgcn_row_order.h: the occupancy order of a structure's rows, built with the graph behind its occupancy words
# (csrc/rgcn_graph.hip).  MODE_ROW_ORDER: RGCN_MODE_ROW_ORDER of that header, one more bit of the option word that
# carries MODE_SPARSE_ROWS - the split NT transforms then take their 64-row tiles in that order.
class RowOrderLayout(ctypes.Structure):
    _fields_ = [(name, c_int64) for name in ("padded_rows", "perm", "row_words", "tile_words", "fin_ptr", "items",
                                              "num_items", "total_words")]


ROW_ORDER_PROTOTYPES = {
    "rgcn_graph_row_order": (c_void_p, [c_void_p, c_int, POINTER(c_int64)]),
    "rgcn_row_order_host": (_I64, [_P, _I64, _I64, _P, POINTER(RowOrderLayout)]),
}
MODE_ROW_ORDER = 4
# rgcn_hip.h: RGCN_MODE_WEIGHT_GRAD / RGCN_MODE_MEAN_GRAD, bits of rgcn_aggregate_ex's option word only - the call
# then computes the gather's adjoint in its edge weights (csrc/edge_grad.hip) instead of gathering.
MODE_WEIGHT_GRAD = 8
MODE_MEAN_GRAD = 16
MODE_LOG_WEIGHT_GRAD = 32          # RGCN_MODE_LOG_WEIGHT_GRAD: through a weighted structure's per-segment normalisation
MODE_EDGE_SUM = 64                 # RGCN_MODE_EDGE_SUM: float[E] by original column in, float[n_key * R] segment sums out

# header of include/ -> its table, in the order the headers arrived: what load() types and every test enumerates
HEADERS = {
    "rgcn_hip.h": PROTOTYPES,
    "rgcn_sampling.h": SAMPLING_PROTOTYPES,
    "rgcn_paths.h": PATHS_PROTOTYPES,
    "rgcn_cluster.h": CLUSTER_PROTOTYPES,
    "rgcn_tsne.h": TSNE_PROTOTYPES,
    "rgcn_neighborhood.h": NEIGHBORHOOD_PROTOTYPES,
    "rgcn_transe.h": TRANSE_PROTOTYPES,
    "rgcn_resample.h": RESAMPLE_PROTOTYPES,
    "rgcn_complex.h": COMPLEX_PROTOTYPES,
    "rgcn_softmax.h": SOFTMAX_PROTOTYPES,
    "rgcn_edge_dropout.h": EDGE_DROPOUT_PROTOTYPES,
    "rgcn_sparse.h": SPARSE_PROTOTYPES,
    "rgcn_row_order.h": ROW_ORDER_PROTOTYPES,
}

_lib = None


class RGCNLibraryError(RuntimeError):
    """The HIP library is missing / unloadable / of the wrong ABI."""


def all_prototypes() -> dict:
    """name -> (restype, argtypes) over every header; a name that two headers' tables hold is refused"""
    merged, owner = {}, {}
    for header, table in HEADERS.items():
        for name, prototype in table.items():
            if name in owner:
                raise RGCNLibraryError(f"{name} is in the tables of both {owner[name]} and {header}")
            merged[name], owner[name] = prototype, header
    return merged


def load() -> ctypes.CDLL:
    """dlopen the library once and type every entry point.  Raises loudly."""
    global _lib
    if _lib is not None:
        return _lib
    prototypes = all_prototypes()
    if not os.path.exists(LIB_PATH):
        raise RGCNLibraryError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `make -C primekg_rgcn_linkprediction_amd/csrc`). There is no "
            f"CPU/PyTorch fallback for the R-GCN path.")
    try:
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    except OSError as exc:  # pragma: no cover - depends on the host
        raise RGCNLibraryError(f"cannot load {LIB_PATH}: {exc}") from exc
    for name, (restype, argtypes) in prototypes.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise RGCNLibraryError(f"{LIB_PATH} does not export {name}") from exc
        fn.restype = restype
        fn.argtypes = argtypes
    got = lib.rgcn_abi_version()
    if got != ABI_VERSION:
        raise RGCNLibraryError(f"{LIB_PATH} has ABI version {got}, host code expects {ABI_VERSION}")
    _lib = lib
    return lib


def available() -> bool:
    try:
        load()
        return True
    except RGCNLibraryError:
        return False


def strerror(code: int) -> str:
    return load().rgcn_strerror(code).decode()


def check(code: int, what: str) -> None:
    """Map a C return code to the Python exception the reference's stack would raise."""
    if code == RGCN_OK:
        return
    msg = f"{what}: {strerror(code)} (code {code})"
    if code == RGCN_ERR_RANGE:
        raise IndexError(msg)
    if code in (RGCN_ERR_ARG, RGCN_ERR_UNSUPPORTED):
        raise ValueError(msg)
    if code == RGCN_ERR_ALIGN:
        raise ValueError(f"{what}: a tensor's base address is not aligned: {strerror(code)} (code {code}). Every tensor "
                         f"torch allocates qualifies, and so do row slices of a table whose width is a multiple of 4; a "
                         f"view that starts some elements into a flat buffer does not - pass tensor.clone()")
    raise RuntimeError(msg)
