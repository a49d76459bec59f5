"""The C surface, every header of ``_lib.HEADERS`` against its ctypes table and the built library (no GPU): the same
functions with the same parameters and return types, exported and typed by ``load()``; no name in two headers; only
``rgcn_hip.h`` forwardable by ``rgcn_sequence_run``; every header plain C; one ABI version in all three places.

``_lib`` never reads a header - the package works without ``include/`` beside it - so the table is the host's statement
and this file holds it to the header.  ``EXPECTED`` pins what each header declares (name: number of parameters): a
function dropped from header AND table at once is still noticed.
"""
import os

import pytest

import c_surface as S
from primekg_rgcn_linkprediction_amd import _lib

HEADERS = list(_lib.HEADERS)
SECONDARY = HEADERS[1:]

EXPECTED = {
    "rgcn_hip.h": {
        "distmult_bce_bwd": 21, "distmult_bce_fwd": 15, "distmult_bce_reduce": 10, "distmult_bwd": 19,
        "distmult_bwd_workspace_bytes": 3, "distmult_fwd": 13, "distmult_rank_masked": 13, "distmult_rank_tails": 9,
        "distmult_score_all_tails": 11, "distmult_topk_masked": 17, "distmult_topk_workspace_bytes": 4,
        "rgcn_abi_version": 0, "rgcn_absmax": 6, "rgcn_absmax_multi": 7, "rgcn_absmax_pack": 14,
        "rgcn_adam_clip_step": 19, "rgcn_adam_workspace_bytes": 2, "rgcn_aggregate": 8, "rgcn_aggregate_deferrable": 3,
        "rgcn_aggregate_ex": 13, "rgcn_aggregate_workspace_bytes": 3, "rgcn_basis_compose": 7,
        "rgcn_basis_compose_bwd": 11, "rgcn_basis_compose_bwd_workspace_bytes": 3, "rgcn_graph_arrays": 6,
        "rgcn_graph_create": 7, "rgcn_graph_create_bipartite": 10, "rgcn_graph_destroy": 1, "rgcn_graph_export": 7,
        "rgcn_graph_import": 13, "rgcn_graph_num_edges": 1, "rgcn_graph_num_levels": 2, "rgcn_graph_num_nodes": 1,
        "rgcn_graph_num_relations": 1, "rgcn_graph_tile_mask": 3, "rgcn_graph_weight_bound": 2,
        "rgcn_index_error_fetch": 2, "rgcn_layer_bwd_input_fused": 20, "rgcn_layer_bwd_input_fused_supported": 3,
        "rgcn_layer_fwd_fused": 18, "rgcn_layer_fwd_fused_supported": 3, "rgcn_rank_allow_bits": 5,
        "rgcn_rank_exclude_bits": 9, "rgcn_sample_batch": 14, "rgcn_segment_sum": 9,
        "rgcn_segment_sum_workspace_bytes": 3, "rgcn_sequence_run": 7, "rgcn_slab_reduce": 2, "rgcn_strerror": 1,
        "rgcn_transform_bwd_input": 12, "rgcn_transform_bwd_input_chain_split": 28,
        "rgcn_transform_bwd_input_chain_supported": 5, "rgcn_transform_bwd_input_split": 24,
        "rgcn_transform_bwd_params": 14, "rgcn_transform_bwd_params_begin": 15,
        "rgcn_transform_bwd_params_split_begin": 20, "rgcn_transform_bwd_params_split_workspace_bytes": 4,
        "rgcn_transform_bwd_params_workspace_bytes": 4, "rgcn_transform_first_split": 13, "rgcn_transform_fwd": 13,
        "rgcn_transform_fwd_f16": 15, "rgcn_transform_fwd_f16_workspace_bytes": 3, "rgcn_transform_fwd_split": 24,
        "rgcn_transform_split_workspace_bytes": 3, "rgcn_weights_split_bytes": 3, "rgcn_weights_split_pack": 8,
        "rgcn_weights_split_pack_multi": 13},
    "rgcn_sampling.h": {"rgcn_sample_batch_constrained": 31},
    "rgcn_paths.h": {"rgcn_edge_cosine": 8, "rgcn_paths_topk": 21, "rgcn_paths_workspace_bytes": 3},
    "rgcn_cluster.h": {"rgcn_kmeans_assign": 13, "rgcn_kmeans_inertia": 11, "rgcn_kmeans_update": 16,
                       "rgcn_kmeans_workspace_bytes": 4, "rgcn_silhouette_samples": 16, "rgcn_silhouette_workspace_bytes": 4},
    "rgcn_tsne.h": {"rgcn_knn_refine": 8, "rgcn_tsne_affinities": 7, "rgcn_tsne_gradient": 15, "rgcn_tsne_update": 12,
                    "rgcn_tsne_workspace_bytes": 2},
    "rgcn_neighborhood.h": {"rgcn_neighborhood_max_nodes": 0, "rgcn_pair_neighborhood": 21},
    "rgcn_transe.h": {"rgcn_transe_step": 17, "rgcn_transe_step_workspace_bytes": 3},
    "rgcn_resample.h": {"rgcn_resample_curves": 15, "rgcn_resample_ranks": 13, "rgcn_resample_weights": 5},
    "rgcn_complex.h": {"complex_bce_bwd": 21, "complex_bce_fwd": 15, "complex_bwd": 19, "complex_bwd_workspace_bytes": 3,
                       "complex_fwd": 13, "rgcn_complex_query": 11},
    "rgcn_softmax.h": {"rgcn_softmax_grad": 19, "rgcn_softmax_lse": 19, "rgcn_softmax_workspace_bytes": 4},
    "rgcn_edge_dropout.h": {"rgcn_edge_dropout_create": 3, "rgcn_edge_dropout_destroy": 1, "rgcn_edge_dropout_draw": 8,
                            "rgcn_edge_dropout_graph": 1, "rgcn_edge_dropout_kept": 1, "rgcn_edge_dropout_kept_export": 3},
    "rgcn_sparse.h": {"rgcn_graph_row_mask": 3, "rgcn_occupancy_host": 5},
    "rgcn_row_order.h": {"rgcn_graph_row_order": 3, "rgcn_row_order_host": 5},
}

# what `main` returns in the plain-C check where the header has something to assert (default: RGCN_OK), and what stands before it
MAIN = {
    "rgcn_hip.h": ("return rgcn_abi_version() == RGCN_ABI_VERSION && rgcn_graph_num_edges(0) == -1 ? RGCN_OK : 1;", ""),
    "rgcn_cluster.h": ("return RGCN_CLUSTER_MAX_K > 32 ? RGCN_OK : 1;", ""),
    "rgcn_tsne.h": ("return RGCN_KNN_MAX_K == 127 ? RGCN_OK : 1;", ""),
    "rgcn_resample.h": ("return t[0] == 1580030168u ? RGCN_OK : 1;",
                        "static const unsigned t[RGCN_RESAMPLE_LEVELS] = RGCN_RESAMPLE_THRESHOLDS;\n"),
}

# words rgcn_hip.h must not contain at all, comments included - wider than the function names, which are all checked
NOT_IN_MAIN_HEADER = ("rgcn_paths", "rgcn_kmeans", "rgcn_silhouette", "rgcn_tsne", "rgcn_knn", "rgcn_resample", "edge_dropout")


def test_the_registry_is_the_headers_of_include_and_the_module_level_tables():
    assert HEADERS[0] == "rgcn_hip.h" and len(HEADERS) == 13 and sorted(HEADERS) == sorted(EXPECTED)
    assert sorted(HEADERS) == sorted(os.listdir(os.path.join(S.ROOT, "include")))
    assert _lib.HEADERS["rgcn_hip.h"] is _lib.PROTOTYPES
    for header in SECONDARY:                       # rgcn_edge_dropout.h -> EDGE_DROPOUT_PROTOTYPES: the same dict object
        assert _lib.HEADERS[header] is getattr(_lib, header[len("rgcn_"):-2].upper() + "_PROTOTYPES"), header
    merged = _lib.all_prototypes()
    assert len(merged) == sum(len(t) for t in _lib.HEADERS.values())
    assert all(merged[name] is proto for table in _lib.HEADERS.values() for name, proto in table.items())


@pytest.mark.parametrize("header", HEADERS)
def test_header_table_and_library_agree(header):
    """names, then per function: parameter count, kind position by position (pointer / float / double / size_t /
    int64_t / int), the return type the header declares, the export, and what load() typed it with.  A ctypes prototype
    that drifts from the header passes a wrong pointer or a truncated size without any error."""
    declared, table, lib = S.declared(header), _lib.HEADERS[header], _lib.load()
    assert sorted(declared) == sorted(table) == sorted(EXPECTED[header]), \
        f"{header}: not in all of header, table and EXPECTED: " + \
        ", ".join(sorted(set(declared) ^ set(table) | set(declared) ^ set(EXPECTED[header])))
    wrong = []
    for name, (returns, params) in declared.items():
        restype, argtypes = table[name]
        if not len(argtypes) == len(params) == EXPECTED[header][name]:
            wrong.append(f"{header}: {name}: {len(params)} parameters declared, {len(argtypes)} in the table, "
                         f"{EXPECTED[header][name]} expected")
            continue
        for i, (param, ty) in enumerate(zip(params, argtypes)):
            if S.kind_in_ctypes(ty) != S.kind_in_header(param):
                wrong.append(f"{header}: {name}: parameter {i} ({param}) is {S.kind_in_ctypes(ty)} in the table")
        if restype is not S.restype_in_header(returns):
            wrong.append(f"{header}: {name}: returns {returns}, the table says {getattr(restype, '__name__', restype)}")
        fn = getattr(lib, name, None)
        if fn is None:
            wrong.append(f"{header}: {name}: not exported by the library")
        elif fn.argtypes != argtypes or fn.restype is not restype:
            wrong.append(f"{header}: {name}: load() typed it ({fn.restype}, {fn.argtypes}), not as the table says")
    assert not wrong, "\n".join(wrong)


def test_no_name_is_in_two_headers_and_only_the_main_header_is_forwardable():
    for what, names_of in (("table", lambda h: set(_lib.HEADERS[h])), ("header", lambda h: set(S.declared(h)))):
        for i, a in enumerate(HEADERS):
            for b in HEADERS[i + 1:]:
                assert not names_of(a) & names_of(b), f"{what}s of {a} and {b} share {sorted(names_of(a) & names_of(b))}"
    assert set(_lib.SEQ_FUNCTIONS) <= set(_lib.PROTOTYPES) and set(_lib.SEQ_HOST_ARRAYS) <= set(_lib.SEQ_FUNCTIONS)
    main = S.header_text("rgcn_hip.h")
    for header in SECONDARY:
        assert '#include "rgcn_hip.h"' in S.header_text(header), header
        for name in _lib.HEADERS[header]:
            assert name not in main, f"rgcn_hip.h mentions {name} of {header}"
    assert not [word for word in NOT_IN_MAIN_HEADER if word in main]


def test_a_name_in_two_tables_is_refused_by_load(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.TSNE_PROTOTYPES, "rgcn_kmeans_assign", _lib.CLUSTER_PROTOTYPES["rgcn_kmeans_assign"])
    with pytest.raises(_lib.RGCNLibraryError, match="rgcn_kmeans_assign.*rgcn_cluster.h.*rgcn_tsne.h"):
        _lib.load()


@pytest.mark.parametrize("header", HEADERS)
def test_header_is_plain_c(header, tmp_path):
    S.plain_c(header, tmp_path, *MAIN.get(header, ()))


def test_one_abi_version_in_the_header_the_binding_and_the_library():
    assert "#define RGCN_ABI_VERSION 38\n" in S.header_text("rgcn_hip.h")
    assert _lib.ABI_VERSION == 38 == _lib.load().rgcn_abi_version()
