"""Filtered / type-constrained ranking, the part that needs no GPU: the C-ABI surface of the three new entry
points, the known-triple CSRs against a brute-force dict of sets, node classes from an ``idx2node`` map, the
committed node-type fixture, the evaluation CLI's new flags."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from primekg_rgcn_linkprediction_amd import _lib, graphio, ops, synth
from primekg_rgcn_linkprediction_amd import evaluate as E


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    A, U, OK = _lib.RGCN_ERR_ARG, _lib.RGCN_ERR_UNSUPPORTED, _lib.RGCN_OK
    # distmult_rank_masked(q, emb, true, target, allow, query_class, classes, exclude, B, N, d, beaten, stream)
    assert lib.distmult_rank_masked(None, None, None, None, None, None, 0, None, 4, 100, 48, None, None) == U    # d % 32
    assert lib.distmult_rank_masked(None, None, None, None, None, None, 0, None, 4, 100, 64, None, None) == A    # nulls
    assert lib.distmult_rank_masked(None, None, None, None, None, None, 0, None, -1, 100, 64, None, None) == A
    assert lib.distmult_rank_masked(None, None, None, None, None, None, 0, None, 4, 0, 64, None, None) == A
    assert lib.distmult_rank_masked(None, None, None, None, None, None, -1, None, 4, 100, 64, None, None) == A
    assert lib.distmult_rank_masked(None, None, None, None, 8, None, 3, None, 4, 100, 64, None, None) == A       # allow, no classes
    assert lib.distmult_rank_masked(None, None, None, None, None, None, 0, None, 0, 100, 64, None, None) == OK   # empty batch
    # rgcn_rank_exclude_bits(ptr, ids, seg, segments, nnz, B, N, exclude, stream)
    assert lib.rgcn_rank_exclude_bits(None, None, None, 3, 5, 4, 100, None, None) == A
    assert lib.rgcn_rank_exclude_bits(None, None, None, 3, 5, -1, 100, None, None) == A
    assert lib.rgcn_rank_exclude_bits(None, None, None, -3, 5, 4, 100, None, None) == A
    assert lib.rgcn_rank_exclude_bits(None, None, None, 3, 5, 4, 0, None, None) == A
    assert lib.rgcn_rank_exclude_bits(None, None, None, 3, 5, 0, 100, None, None) == OK
    assert lib.rgcn_rank_exclude_bits(None, None, 8, 3, 5, 4, 1 << 31, 8, None) == A                             # CSR arrays missing
    # rgcn_rank_allow_bits(class_of, N, classes, allow, stream)
    assert lib.rgcn_rank_allow_bits(None, 100, 3, None, None) == A
    assert lib.rgcn_rank_allow_bits(8, 0, 3, 8, None) == A
    assert lib.rgcn_rank_allow_bits(8, 100, 0, 8, None) == A
    assert lib.rgcn_rank_allow_bits(8, 1 << 31, 3, 8, None) == U


def _brute(edge_index, edge_type):
    tails, heads = {}, {}
    for (h, t), r in zip(edge_index.t().tolist(), edge_type.tolist()):
        tails.setdefault((h, r), set()).add(t)
        heads.setdefault((t, r), set()).add(h)
    return {"tail": tails, "head": heads}


def test_known_triples_on_cpu_against_a_dict_of_sets():
    gen = torch.Generator().manual_seed(3)
    n, r = 40, 3
    ei = torch.randint(0, 30, (2, 400), generator=gen)          # nodes 30..39 never occur
    et = torch.randint(0, 2, (400,), generator=gen)             # relation 2 has no edge
    ei, et = torch.cat([ei, ei[:, :50]], 1), torch.cat([et, et[:50]])           # duplicate edges
    known = ops.KnownTriples(ei, et, n, r)
    want = _brute(ei, et)
    for side in ("tail", "head"):
        keys, ptr, ids = known.csr(side)
        assert ptr[0] == 0 and ptr[-1] == ids.numel() == sum(len(s) for s in want[side].values())   # duplicates collapsed
        assert keys.numel() == len(want[side]) and bool((keys[1:] > keys[:-1]).all())
        anchors = torch.arange(n).repeat_interleave(r)
        rels = torch.arange(r).repeat(n)
        seg = known.segments(side, anchors, rels)
        for a, rel, s in zip(anchors.tolist(), rels.tolist(), seg.tolist()):
            if (a, rel) not in want[side]:
                assert s == -1                                  # an (h, r) without edges, an anchor that never occurs
            else:
                assert sorted(want[side][(a, rel)]) == ids[ptr[s]: ptr[s + 1]].tolist()
        assert (seg[anchors >= 30] == -1).all() and (seg[rels == 2] == -1).all() and (seg >= 0).any()
    # an id outside its range aliases no other anchor's key (1 * 3 + 3 == 2 * 3 + 0): nothing known
    assert known.segments("tail", torch.tensor([2, 1, 40, -1]), torch.tensor([0, 3, 0, 0])).tolist()[1:] == [-1, -1, -1]
    empty = ops.KnownTriples(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), n, r)
    assert empty.segments("tail", torch.tensor([1, 2]), torch.tensor([0, 1])).tolist() == [-1, -1]
    with pytest.raises(IndexError):
        ops.KnownTriples(torch.tensor([[0], [40]]), torch.tensor([0]), n, r)
    with pytest.raises(ValueError):
        known.segments("both", anchors, rels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the bit mask itself is a kernel
        known.exclude_bits("tail", anchors, rels)


def test_node_classes_drop_the_rows_past_num_nodes():
    # (id, name, type) triples sorted by type; two aliases make idx2node longer than the graph has nodes
    idx2node = {0: ("7", "a", "disease"), 1: ("9", "b", "disease"), 2: ("1", "c", "drug"), 3: ("3", "d", "gene/protein"),
                4: ("4", "e", "gene/protein"), 5: ("4", "e-alias", "gene/protein"), 6: ("5", "f", "gene/protein")}
    classes, names = graphio.node_classes(idx2node, 5)
    assert names == ["disease", "drug", "gene/protein"] and classes.dtype == torch.int32
    assert classes.tolist() == [0, 0, 1, 2, 2]
    classes, names = graphio.node_classes(idx2node, 2)          # class ids by sorted name of the types that occur
    assert names == ["disease"] and classes.tolist() == [0, 0]
    with pytest.raises(ValueError):
        graphio.node_classes(idx2node, 8)


def test_committed_node_type_fixture_and_the_synthetic_layout():
    with np.load(os.path.join(GOLDEN, "primekg_node_types.npz"), allow_pickle=False) as raw:   # (holds a string array)
        assert raw["class_names"].tolist() == ["disease", "drug", "gene/protein"] and int(raw["num_nodes"]) == 30926
        cls = torch.from_numpy(raw["node_class"].copy())
    assert cls.shape == (30926,) and cls.dtype == torch.int8
    assert torch.bincount(cls.long()).tolist() == [5593, 6282, 19051]           # disease / drug / gene-protein
    assert bool((cls[1:] >= cls[:-1]).all())                                    # ids are type-sorted in that order
    synth_cls = synth.primekg_like_node_classes()
    assert synth_cls.dtype == torch.int32 and torch.equal(synth_cls, cls.to(torch.int32))
    # the real test edges: all drug-gene (relation 0), half stored drug -> gene and half gene -> drug
    t = load_golden("primekg_test_edges.npz")
    ei = t["edge_index"].long()
    assert ei.shape == (2, 15372) and int(t["edge_type"].abs().max()) == 0
    pairs = cls[ei[0]].long() * 3 + cls[ei[1]].long()
    assert int((pairs == 1 * 3 + 2).sum()) == 7686 and int((pairs == 2 * 3 + 1).sum()) == 7686


def test_cli_flags_and_node_type_files(tmp_path, capsys):
    base = ["--model_path", "m.pt"]
    args = E.parse_args(base)
    assert not (args.filtered or args.type_constrained or args.both_sides) and args.node_types is None
    args = E.parse_args(base + ["--filtered", "--both_sides"])
    assert args.filtered and args.both_sides and not args.type_constrained
    args = E.parse_args(base + ["--filtered", "--type_constrained", "--both_sides", "--node_types", "x.npz"])
    assert args.type_constrained and args.node_types == "x.npz"
    with pytest.raises(SystemExit):
        E.parse_args(base + ["--type_constrained"])
    assert "--node_types" in capsys.readouterr().err
    # the three file forms of --node_types
    idx2node = {0: ("7", "a", "disease"), 1: ("1", "c", "drug"), 2: ("3", "d", "gene/protein"), 3: ("3", "alias", "gene/protein")}
    torch.save({"node2idx": {("7", "disease"): 0, ("1", "drug"): 1, ("3", "gene/protein"): 3}, "idx2node": idx2node,
                "relation2idx": {"drug_gene": 0}, "idx2relation": {0: "drug_gene"}}, tmp_path / "mappings.pt")
    assert E.load_node_classes(str(tmp_path / "mappings.pt"), 3).tolist() == [0, 1, 2]
    np.savez(tmp_path / "c.npz", node_class=np.array([2, 0, 1], dtype=np.int8))
    got = E.load_node_classes(str(tmp_path / "c.npz"), 3)
    assert got.dtype == torch.int32 and got.tolist() == [2, 0, 1]
    torch.save(torch.tensor([1, 1, 0]), tmp_path / "c.pt")
    assert E.load_node_classes(str(tmp_path / "c.pt"), 3).tolist() == [1, 1, 0]
    with pytest.raises(ValueError):
        E.load_node_classes(str(tmp_path / "c.pt"), 4)


def test_type_constrained_without_node_classes_is_a_clear_error():
    from primekg_rgcn_linkprediction_amd import DrugDiseaseModel
    data = {"edge_index": torch.tensor([[0, 1], [1, 0]]), "edge_type": torch.tensor([0, 0]), "num_nodes": 4,
            "num_relations": 1}
    ev = E.ModelEvaluator(DrugDiseaseModel(4, 1, 32, 32), data, data, torch.device("cpu"))
    with pytest.raises(ValueError, match="node classes"):
        ev._protocol(False, True)
    known = ev.known_triples()                                   # full graph united with the test triples, once
    assert known is ev.known_triples() and known.csr("tail")[2].tolist() == [1, 0]
