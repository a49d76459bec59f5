"""The alignment contract of the C boundary, the part that needs no GPU (``include/rgcn_hip.h``, "Alignment").

Every entry point refuses a pointer below the alignment its kernels need with ``RGCN_ERR_ALIGN`` - after every other
argument check and before its first HIP runtime call.  For each entry point ``CASES`` holds one argument set (a few have
two) that passes every other check at the smallest legal sizes, with fake, well-aligned device addresses and the
workspace size the entry's own ``*_workspace_bytes`` returns.  One pointer at a time is then moved below its alignment
and the call must return exactly ``RGCN_ERR_ALIGN``: because the check sits last, that code also says the rest of the
set was accepted; were the check missing, the call would go on to the HIP runtime, which fails here (``RGCN_ERR_HIP``).
The fully aligned set is never called - that would be a launch.

The alignment of a parameter is the ``Dev(...)`` of its position: the table of this test, in the notation of
``c_surface.py``.  ``CASES`` covers ``rgcn_hip.h`` and the headers that arrived before the contract did; the resample,
ComplEx and softmax host tests keep the rows of their own headers.  ``test_every_pointer_parameter_has_a_row`` walks
every prototype of every header of ``_lib.HEADERS`` through all of them: a pointer parameter has a row, or stands by name
in ``WITHOUT_ALIGNMENT_ROW`` - which must list exactly the ones without - so a new entry point cannot be added unnoticed.
"""
import ctypes
import math

import pytest

import c_surface as S
from c_surface import FAKE_BASE, FAKE_STEP, GRAPH, HANDLE, STREAM, T4, T8, T16, Dev, DevArray, Host, Job, _q, i64s
from primekg_rgcn_linkprediction_amd import _lib

NINF = -math.inf
OUT_HANDLE = Host(lambda: ctypes.pointer(ctypes.c_void_p()))
EMPTY_JOB = Host(lambda: ctypes.pointer(_lib.SlabJob()))


def test_the_fake_handle_reads_back_through_the_library():
    """the mirror above has the layout the library was built with: every accessor returns what was put in"""
    lib = _lib.load()
    assert lib.rgcn_graph_num_edges(GRAPH) == 1 and lib.rgcn_graph_num_nodes(GRAPH) == 1
    assert lib.rgcn_graph_num_relations(GRAPH) == 1
    assert lib.rgcn_graph_num_levels(GRAPH, 0) == 2 and lib.rgcn_graph_num_levels(GRAPH, 1) == 0
    assert lib.rgcn_graph_weight_bound(GRAPH, 0) == 1.0 and lib.rgcn_graph_weight_bound(GRAPH, 1) == 0.0
    assert lib.rgcn_aggregate_workspace_bytes(GRAPH, 0, 4) == 16 and lib.rgcn_aggregate_workspace_bytes(GRAPH, 1, 4) == 0
    got = [ctypes.c_void_p() for _ in range(4)]
    assert lib.rgcn_graph_arrays(GRAPH, 0, *[ctypes.byref(p) for p in got]) == _lib.RGCN_OK
    assert [p.value for p in got] == [FAKE_BASE - (i + 1) * FAKE_STEP for i in range(4)]
    tiles = ctypes.c_int64(-1)
    assert lib.rgcn_graph_tile_mask(GRAPH, 0, ctypes.byref(tiles)) is None and tiles.value == 0
    assert lib.rgcn_aggregate_deferrable(GRAPH, 0, 64) == 0


# ------------------------------------------------------------------------------------------------ the table
# name -> argument sets, parameter by parameter: an int / float / callable (evaluated) is passed as it is
CASES = {
    # --- surface without device pointers of the caller's
    "rgcn_abi_version": [[]],
    "rgcn_strerror": [[0]],
    "rgcn_graph_destroy": [[HANDLE]],
    "rgcn_graph_num_edges": [[HANDLE]],
    "rgcn_graph_num_nodes": [[HANDLE]],
    "rgcn_graph_num_relations": [[HANDLE]],
    "rgcn_graph_num_levels": [[HANDLE, 0]],
    "rgcn_graph_weight_bound": [[HANDLE, 0]],
    "rgcn_graph_arrays": [[HANDLE, 0, Host(), Host(), Host(), Host()]],
    "rgcn_graph_tile_mask": [[HANDLE, 0, Host()]],
    "rgcn_aggregate_workspace_bytes": [[HANDLE, 0, 4]],
    "rgcn_aggregate_deferrable": [[HANDLE, 0, 4]],
    "rgcn_adam_workspace_bytes": [[1, Host()]],
    "rgcn_index_error_fetch": [[Host(), STREAM]],
    "rgcn_sequence_run": [[Host(), 0, Host(), 0, Host(), 0, STREAM]],     # its calls pass through the entries below
    # --- graph structure: index columns and CSR arrays, one element at a time
    "rgcn_graph_create": [[T8, T8, 1, 1, 1, STREAM, OUT_HANDLE]],
    "rgcn_graph_create_bipartite": [[T8, T8, T8, 1, 1, 1, 1, T4, STREAM, OUT_HANDLE]],
    "rgcn_graph_export": [[HANDLE, 0, T4, T4, T8, T4, STREAM]],
    "rgcn_graph_import": [[1, 1, 1, T4, T4, T8, T4, T4, T4, T8, T4, STREAM, OUT_HANDLE]],
    # --- gathers
    "rgcn_aggregate": [[HANDLE, 0, T16, 4, T16, T16, 16, STREAM]],
    "rgcn_aggregate_ex": [[HANDLE, 0, T16, 0, 4, T16, T16, 16, 0, -1, Job(), T4, STREAM],
                          [HANDLE, 0, Dev(16, half=True), 1, 8, T16, T16, 32, 0, -1, Job(), None, STREAM]],
    # --- fp32 and fp16 transforms
    "rgcn_transform_fwd": [[T16, T16, T16, T16, T16, 1, T4, 1, 1, 4, 4, T16, STREAM]],
    "rgcn_transform_fwd_f16_workspace_bytes": [[1, 32, 4]],
    "rgcn_transform_fwd_f16": [[T16, T16, T16, T16, T16, 1, T4, 1, 1, 32, 4, T16, T16,
                                _q("rgcn_transform_fwd_f16_workspace_bytes", 1, 32, 4), STREAM]],
    "rgcn_transform_bwd_input": [[T16, T16, T16, T16, T16, T4, 1, 1, 4, 4, T16, STREAM]],
    "rgcn_transform_bwd_params_workspace_bytes": [[1, 1, 4, 4]],
    "rgcn_transform_bwd_params": [[T16, T16, T16, T4, 1, 1, 4, 4, T16, T16, T16, T16,
                                   _q("rgcn_transform_bwd_params_workspace_bytes", 1, 1, 4, 4), STREAM]],
    "rgcn_transform_bwd_params_begin": [[T16, T16, T16, T4, 1, 1, 4, 4, T16, T16, T16, T16,
                                         _q("rgcn_transform_bwd_params_workspace_bytes", 1, 1, 4, 4), STREAM, EMPTY_JOB]],
    "rgcn_slab_reduce": [[Job(), STREAM]],
    # --- operand maxima and split weights
    "rgcn_absmax": [[T16, 1, T4, T4, 1, STREAM]],
    "rgcn_absmax_multi": [[2, DevArray(T16, 2), i64s(1, 1), DevArray(T4, 2), T4, 1, STREAM]],
    "rgcn_weights_split_bytes": [[1, 4, 4]],
    "rgcn_absmax_pack": [[T16, 1, T4, T4, 1, 1, DevArray(T16), DevArray(T16), i64s(1), i64s(4), i64s(4), DevArray(T16),
                          Host(lambda: (ctypes.c_size_t * 1)(_lib.load().rgcn_weights_split_bytes(1, 4, 4))), STREAM]],
    "rgcn_weights_split_pack_multi": [[1, DevArray(T16), DevArray(T16), i64s(1), i64s(4), i64s(4), DevArray(T4), DevArray(T4),
                                       DevArray(T16),
                                       Host(lambda: (ctypes.c_size_t * 1)(_lib.load().rgcn_weights_split_bytes(1, 4, 4))),
                                       T4, 1, STREAM]],
    "rgcn_weights_split_pack": [[T16, T16, 1, 4, 4, T16, _q("rgcn_weights_split_bytes", 1, 4, 4), STREAM]],
    # --- split-precision transforms
    "rgcn_transform_split_workspace_bytes": [[1, 32, 4]],
    "rgcn_transform_fwd_split": [[T16, T16, T16, T16, T16, T16, 1, T4, 1, 1, 32, 4, T4, 1.0, T4, 0, T16, T4, T16,
                                  _q("rgcn_transform_split_workspace_bytes", 1, 32, 4), STREAM, HANDLE, 0, T16]],
    "rgcn_transform_bwd_input_split": [[T16, T16, T16, T16, T16, T16, T4, 1, 1, 4, 32, T4, 1.0, T4, 0, T16, T4, T16,
                                        _q("rgcn_transform_split_workspace_bytes", 1, 4, 32), STREAM, HANDLE, 0, T16, 1.0]],
    "rgcn_transform_bwd_input_chain_supported": [[1, 128, 32, 1, 4]],
    "rgcn_transform_bwd_input_chain_split": [[T16, T16, T16, T16, T16, T16, T4, 1, 1, 128, 32, T4, 1.0, T4, T16, T4, T16,
                                              _q("rgcn_transform_split_workspace_bytes", 1, 128, 32), STREAM, HANDLE, 0, T16,
                                              1.0, T16, 1, 1, 4, T16]],
    "rgcn_transform_first_split": [[T16, T16, 1, 1, 1, 4, 32, T4, 0, T16, T16, 1 << 16, STREAM]],
    "rgcn_transform_bwd_params_split_workspace_bytes": [[1, 1, 64, 4]],
    "rgcn_transform_bwd_params_split_begin": [[T16, T16, T16, T4, 1, 1, 64, 4, T4, 1.0, T4, T4, 0, T16, T16, T16, T16,
                                               _q("rgcn_transform_bwd_params_split_workspace_bytes", 1, 1, 64, 4), STREAM,
                                               EMPTY_JOB]],
    # --- fused layers: CSR ids, weights, occupancy words and amax heads go one word at a time
    "rgcn_layer_fwd_fused_supported": [[1, 64, 128]],
    "rgcn_layer_fwd_fused": [[T4, T4, T4, 1, 1, T16, T16, T16, 1, T16, 1, 64, 128, T4, T16, T4, T16, STREAM]],
    "rgcn_layer_bwd_input_fused_supported": [[1, 64, 64]],
    "rgcn_layer_bwd_input_fused": [[T4, T4, T4, T4, 1, 1, T16, T16, T16, 1, T16, 64, 64, T4, 1.0, T16, T4, STREAM, 1.0, T4]],
    # --- DistMult head: tables by float4 rows, per-sample vectors and scalars one element at a time
    "distmult_fwd": [[T16, T8, 1, T16, T8, 1, T16, T8, 1, 1, 4, T4, STREAM]],
    "distmult_bce_fwd": [[T16, T8, 1, T16, T8, 1, T16, T8, 1, T4, 1, 4, T4, T4, STREAM]],
    "distmult_bce_reduce": [[T4, T4, T4, 1, T4, T8, T8, T8, 1, STREAM]],
    "distmult_bwd_workspace_bytes": [[1, 4, 1]],
    "distmult_bwd": [[T4, T16, T8, 1, T16, T8, 1, T16, T8, 1, 1, 4, T16, T16, T16, T16,
                      _q("distmult_bwd_workspace_bytes", 1, 4, 1), 1, STREAM]],
    "distmult_bce_bwd": [[T4, T4, T4, T16, T8, 1, T16, T8, 1, T16, T8, 1, 1, 4, T16, T16, T16, T16,
                          _q("distmult_bwd_workspace_bytes", 1, 4, 1), 1, STREAM]],
    "rgcn_segment_sum_workspace_bytes": [[1, 4, 1]],
    "rgcn_segment_sum": [[T16, T8, 1, 4, 1, T16, T16, _q("rgcn_segment_sum_workspace_bytes", 1, 4, 1), STREAM]],
    "rgcn_sample_batch": [[T8, T8, 1, T8, T8, 1, 1, 1, T8, T8, T8, T8, T4, STREAM]],
    # --- ranking, masks, top-k, the score matrix
    "distmult_rank_tails": [[T16, T16, T4, T8, 1, 1, 32, T4, STREAM]],
    "distmult_rank_masked": [[T16, T16, T4, T8, T4, T4, 1, T4, 1, 1, 32, T4, STREAM]],
    "rgcn_rank_exclude_bits": [[T8, T8, T8, 1, 1, 1, 1, T4, STREAM]],
    "rgcn_rank_allow_bits": [[T4, 1, 1, T4, STREAM]],
    "distmult_topk_workspace_bytes": [[1, 1, 1, 0]],
    "distmult_topk_masked": [[T16, T16, T4, T4, 1, T4, NINF, 1, 1, 32, 1, 0, T8, T4, T16,
                              _q("distmult_topk_workspace_bytes", 1, 1, 1, 0), STREAM]],
    "distmult_score_all_tails": [[T16, T16, T8, 1, T16, 1, 1, 32, T16, T4, STREAM]],
    # --- basis composition: the coefficients are read one at a time
    "rgcn_basis_compose": [[T4, T16, 1, 1, 4, T16, STREAM]],
    "rgcn_basis_compose_bwd_workspace_bytes": [[1, 1, 4]],
    "rgcn_basis_compose_bwd": [[T16, T4, T16, 1, 1, 4, T4, T16, T16, _q("rgcn_basis_compose_bwd_workspace_bytes", 1, 1, 4),
                                STREAM]],
    # --- clip + Adam: its kernels choose the access by alignment themselves, so everything is at 4
    "rgcn_adam_clip_step": [[2, DevArray(T4, 2), DevArray(T4, 2), DevArray(T4, 2), DevArray(T4, 2), DevArray(T4, 2),
                             i64s(1, 1), 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, T4, DevArray(T4, 2), T4, 8, STREAM]],
    # --- include/rgcn_sampling.h
    "rgcn_sample_batch_constrained": [[T8, T8, 1, T8, T8, 1, 1, 1, T8, T4, T8, T8, 1, T8, T8, T8, 1, 1, T8, T8, T8, 1, 1, 1, 1,
                                       T8, T8, T8, T8, T4, STREAM]],
    # --- include/rgcn_paths.h
    "rgcn_edge_cosine": [[T16, 1, 32, T8, T4, 1, T4, STREAM]],
    "rgcn_paths_workspace_bytes": [[1, 1, 1]],
    "rgcn_paths_topk": [[T8, T4, T4, T8, T4, T8, 1, 1, T8, T8, 1, 1, 1, 1, T4, T4, T4, T8, T16,
                         _q("rgcn_paths_workspace_bytes", 1, 1, 1), STREAM]],
    # --- include/rgcn_cluster.h
    "rgcn_kmeans_workspace_bytes": [[2, 32, 1, 2]],
    "rgcn_kmeans_assign": [[T16, 2, 32, T16, 1, 2, T4, T4, T4, T4, T16, _q("rgcn_kmeans_workspace_bytes", 2, 32, 1, 2), STREAM]],
    "rgcn_kmeans_update": [[T16, 2, 32, T16, 1, 2, T4, T4, T4, T4, T4, T4, 0.0, T16,
                            _q("rgcn_kmeans_workspace_bytes", 2, 32, 1, 2), STREAM]],
    "rgcn_kmeans_inertia": [[T16, 2, 32, T16, 1, 2, T4, T8, T16, _q("rgcn_kmeans_workspace_bytes", 2, 32, 1, 2), STREAM]],
    "rgcn_silhouette_workspace_bytes": [[2, 128, 2, 0]],
    "rgcn_silhouette_samples": [[T16, T16, T4, T4, T4, T4, 2, 128, 32, 2, 0, T4, T8, T16,
                                 _q("rgcn_silhouette_workspace_bytes", 2, 128, 2, 0), STREAM]],
    # --- include/rgcn_tsne.h: the layout and its gradient are float2 points in the gradient, coordinates in the update
    "rgcn_knn_refine": [[T16, 2, 4, T8, 1, T4, T4, STREAM]],
    "rgcn_tsne_affinities": [[T4, 1, 2, 1.5, T4, T4, STREAM]],
    "rgcn_tsne_workspace_bytes": [[2, 0]],
    "rgcn_tsne_gradient": [[T8, 2, T4, T4, T4, 1, 1.0, 0, 0, T8, T8, T8, T16, _q("rgcn_tsne_workspace_bytes", 2, 0), STREAM]],
    "rgcn_tsne_update": [[T4, 2, 0.5, 1.0, 0.01, T4, T4, T4, T8, T16, _q("rgcn_tsne_workspace_bytes", 2, 0), STREAM]],
    # --- include/rgcn_neighborhood.h: index and count vectors only
    "rgcn_neighborhood_max_nodes": [[]],
    "rgcn_pair_neighborhood": [[T8, T4, T8, T4, 1, 1, T8, T8, 1, 1, T4, 1, 1, T8, T4, T8, T8, T8, T8, T4, STREAM]],
    # --- include/rgcn_transe.h
    "rgcn_transe_step_workspace_bytes": [[1, 4, 1]],
    "rgcn_transe_step": [[T16, 1, T16, 1, 4, T8, T8, T8, 1, 0.1, 1.0, T4, T8, T8, T16,
                          _q("rgcn_transe_step_workspace_bytes", 1, 4, 1), STREAM]],
}

ALIGNMENT_CASES = CASES                # what c_surface.alignment_rows() collects from this module

# pointer parameters that no argument set describes, by function or (function, position): each one a gap in what the
# refusal tests cover, not a statement that the entry point needs no alignment
WITHOUT_ALIGNMENT_ROW = {
    "rgcn_resample_weights": "its one output is bytes; the size refusals of test_resample_host.py call it, no set moves it",
    ("rgcn_softmax_lse", 14): "the optional per-sample loss output is NULL in every set of test_softmax_host.py",
    ("rgcn_softmax_lse", 15): "the optional hit-count output is NULL in every set of test_softmax_host.py",
    "rgcn_edge_dropout_create": "handles, a stream and an out-parameter: no device pointer of the caller's",
    "rgcn_edge_dropout_destroy": "a handle",
    "rgcn_edge_dropout_graph": "a handle",
    "rgcn_edge_dropout_kept": "a handle",
    "rgcn_edge_dropout_kept_export": "its int32 output has no row; the call is only refused for a NULL handle so far",
    "rgcn_edge_dropout_draw": "rng, cursor, position and stats have no row; its checks past the NULLs need a real handle",
    "rgcn_graph_row_mask": "a handle and a host out-parameter",
    "rgcn_occupancy_host": "host arrays only: no device is touched",
    "rgcn_graph_row_order": "a handle and a host out-parameter",
    "rgcn_row_order_host": "host arrays only: no device is touched",
}
_DESCRIBED = (Dev, DevArray, Job, Host)


def test_every_pointer_parameter_has_a_row():
    rows, prototypes = S.alignment_rows(), _lib.all_prototypes()
    assert set(rows) <= set(prototypes), sorted(set(rows) - set(prototypes))
    without = set()
    for name, (_, argtypes) in prototypes.items():
        if name not in rows:
            if any(S.is_pointer(ty) for ty in argtypes):
                without.add(name)
            continue
        for args in rows[name]:
            assert len(args) == len(argtypes), name
        for pos, ty in enumerate(argtypes):
            column = [args[pos] for args in rows[name]]
            if S.is_pointer(ty):
                # None: the optional operand is absent from that set; at least one set must say what the pointer is
                assert all(r is None or isinstance(r, _DESCRIBED) or r in (HANDLE, STREAM) for r in column), (name, pos)
                if all(r is None for r in column):
                    without.add((name, pos))
            else:
                assert all(callable(r) or isinstance(r, (int, float)) for r in column), (name, pos)
    assert without == set(WITHOUT_ALIGNMENT_ROW), sorted(map(str, without ^ set(WITHOUT_ALIGNMENT_ROW)))
    assert all(reason for reason in WITHOUT_ALIGNMENT_ROW.values())


def test_clip_and_adam_stays_at_natural_alignment():
    """its kernels choose float4 or element-wise access by alignment (the existing GPU test runs it 4 bytes into a
    buffer): every tensor, the norm and the workspace are rows of 4"""
    (args,) = CASES["rgcn_adam_clip_step"]
    devs = [a.dev if isinstance(a, DevArray) else a for a in args if isinstance(a, (Dev, DevArray))]
    assert len(devs) == 8 and all(d.align == 4 for d in devs)


# ------------------------------------------------------------------------------------------------ the refusals
def _hub_handle(args, name):
    """the optional hub_graph of the split transforms stays NULL (nothing deferred); every other handle is the fake one"""
    return [None if (a == HANDLE and name.startswith("rgcn_transform_")) else a for a in args]


REFUSALS = [(name, k) for name in sorted(CASES) for k, args in enumerate(CASES[name]) if S.targets(name, args)]


@pytest.mark.parametrize("name,k", REFUSALS, ids=[f"{n}-{k}" if k else n for n, k in REFUSALS])
def test_a_pointer_below_its_alignment_is_refused(name, k):
    failed = S.misaligned_refusals(getattr(_lib.load(), name), name, _hub_handle(CASES[name][k], name))
    assert not failed, "; ".join(failed)


def test_the_entries_with_checks_are_all_the_entries_with_device_pointers():
    """every entry point that takes a device pointer of the caller's is in the refusal table (86 prototypes in this module's
    CASES, 53 with one)"""
    with_pointers = {n for n, _ in REFUSALS}
    without = set(CASES) - with_pointers
    assert len(CASES) == 86 and len(with_pointers) == 53
    assert all(n.endswith(("_bytes", "_supported", "_deferrable", "_max_nodes")) or n.startswith("rgcn_graph_")
               or n in ("rgcn_abi_version", "rgcn_strerror", "rgcn_index_error_fetch", "rgcn_sequence_run") for n in without), without
    assert {"rgcn_graph_create", "rgcn_graph_create_bipartite", "rgcn_graph_import", "rgcn_graph_export"} <= with_pointers


# ------------------------------------------------------------------------------------------------ the Python level
def test_check_raises_a_value_error_that_states_the_rule():
    assert _lib.RGCN_ERR_ALIGN == -6 and _lib.ABI_VERSION >= 36
    text = _lib.strerror(_lib.RGCN_ERR_ALIGN)
    assert "unknown" not in text and "16-byte" in text and "element size" in text
    with pytest.raises(ValueError) as err:
        _lib.check(_lib.RGCN_ERR_ALIGN, "rgcn_aggregate")
    msg = str(err.value)
    assert "rgcn_aggregate" in msg and "base address is not aligned" in msg and ".clone()" in msg and "16-byte" in msg
    assert "(code -6)" in msg
