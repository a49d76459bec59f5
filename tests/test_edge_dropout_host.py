"""CPU tier of edge dropout and hidden batch edges (``include/rgcn_edge_dropout.h``, ``csrc/edge_dropout.hip``,
``ops.EdgeDropout``, ``train.py --edge_dropout / --hide_batch_edges``): the C surface, the argument checks that run
before a launch, the host restatement of the draw (``edge_dropout_reference.py``) against the oracle layer on the kept
subgraph, and the trainer's refusals."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import c_surface as S
import edge_dropout_reference as R
import resample_reference as RR
from conftest import ROOT
from oracle import rgcn_oracle as O
from primekg_rgcn_linkprediction_amd import _lib, train

FAKE = S.FAKE_BASE               # a fake address, never dereferenced


# ---------------------------------------------------------------------------------- C surface
def test_header_table_and_library_agree():
    """names, parameters, return types and exports: test_c_surface.py, for every header.  Here: the Philox stream of the
    draw, in the header, the restatement and the binding, and the build list"""
    header = S.header_text("rgcn_edge_dropout.h")
    stream = int(re.search(r"#define RGCN_EDGE_DROPOUT_STREAM (0x[0-9A-Fa-f]+)u", header).group(1), 16)
    assert stream == R.STREAM == _lib.EDGE_DROPOUT_STREAM != RR.STREAM
    makefile = open(os.path.join(ROOT, "primekg_rgcn_linkprediction_amd", "csrc", "Makefile")).read()
    assert " edge_dropout.hip" in makefile


def test_argument_checks_run_before_any_launch():
    lib = _lib.load()
    out = ctypes.c_void_p(1)
    assert lib.rgcn_edge_dropout_create(None, None, ctypes.byref(out)) == _lib.RGCN_ERR_ARG and out.value is None
    assert lib.rgcn_edge_dropout_create(FAKE, None, None) == _lib.RGCN_ERR_ARG
    assert lib.rgcn_edge_dropout_graph(None) is None and lib.rgcn_edge_dropout_kept(None) is None
    assert lib.rgcn_edge_dropout_kept_export(None, FAKE, None) == _lib.RGCN_ERR_ARG
    lib.rgcn_edge_dropout_destroy(None)
    # a handle that is not a square graph with a mean forward and a weighted transposed direction: refused, untouched
    assert lib.rgcn_edge_dropout_create(S.GRAPH, None, ctypes.byref(out)) == _lib.RGCN_ERR_UNSUPPORTED and out.value is None
    # draw: NULL handle / rng first; the other checks need a handle and run on the GPU tier
    assert lib.rgcn_edge_dropout_draw(None, 0.5, FAKE, None, 0, None, None, None) == _lib.RGCN_ERR_ARG


# ---------------------------------------------------------------------------------- the restatement
def _graph(seed, n=37, r=3, e=700):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=gen)
    et = torch.randint(0, r, (e,), generator=gen)
    ei[1, :120] = 5                                   # a long segment, duplicates, self loops; node n - 1 has no in-edge
    et[:120] = 1
    ei[:, 130:140] = ei[:, 120:130]
    ei[0, 140:150] = ei[1, 140:150]
    ei[1][ei[1] == n - 1] = 0
    return ei, et, n, r


def test_philox_is_the_samplers_generator():
    # the numpy generator the restatement imports against the scalar one, on this header's counter layout
    w = R.words(50, seed=(7 << 32) | 9, epoch=3, c0=1 << 33 | 5)
    for e in (0, 1, 17, 49):
        assert int(w[e]) == RR.philox4x32_10((e, 5, 3, R.STREAM), (9, 7))[0]


@pytest.mark.parametrize("p,window", [(0.0, None), (0.4, None), (0.4, (64, 100)), (0.9, (650, 100))])
def test_weighted_aggregate_is_the_oracle_layer_on_the_kept_subgraph(p, window):
    ei, et, n, r = _graph(1)
    e = ei.size(1)
    gen = torch.Generator().manual_seed(2)
    order = torch.randperm(e, generator=gen)
    position = torch.empty(e, dtype=torch.int64)
    position[order] = torch.arange(e)
    c0, batch = window or (0, 0)
    kept, hidden = R.kept_mask(e, p, seed=1234, epoch=1, c0=c0, batch=batch, position=position.numpy() if window else None)
    if window:                                        # exactly the batch's columns are hidden - a clipped window its rest
        assert sorted(np.nonzero(hidden)[0].tolist()) == sorted(order[c0:c0 + batch].tolist())
    w = R.weights(ei.numpy(), et.numpy(), kept, n, r)
    k = R.kept_counts(ei.numpy(), et.numpy(), kept, n, r)
    assert int(k.sum()) == int(kept.sum()) and w.dtype == np.float32 and bool((w[~kept] == 0).all())
    x = torch.randn(n, 8, generator=gen, dtype=torch.float64)
    ek, tk = (torch.from_numpy(a) for a in R.kept_subgraph(ei.numpy(), et.numpy(), kept))
    # both directions against float64 means over the kept subgraph (the layer's aggregate and its adjoint)
    cnt = O._segment_counts(ek, tk, n, r, torch.float64)
    for transposed, want in ((False, O._mean_agg(x, ek, tk, n, r, cnt)), (True, O._mean_agg_transposed(x, ek, tk, n, r, cnt))):
        got, mag = R.aggregate_f64(x.numpy(), ei.numpy(), et.numpy(), w, n, r, transposed)
        # w = fl32(1 / k): every term carries one float32 rounding of the weight, nothing else differs
        assert bool((np.abs(got - want.numpy()) <= 2.0 ** -23 * mag + 1e-300).all())
    # and the layer: the restated aggregate through the oracle's transform equals the oracle layer on the kept subgraph
    weight, root, bias = (torch.randn(s, generator=gen, dtype=torch.float64) for s in ((r, 8, 4), (8, 4), (4,)))
    agg = torch.from_numpy(R.aggregate_f64(x.numpy(), ei.numpy(), et.numpy(), w, n, r)[0])
    got = agg @ weight.reshape(r * 8, 4) + x @ root + bias
    for ref in (O.rgcn_conv_ref(x, ek, tk, weight, root, bias), O.rgcn_conv_dense_f64(x, ek, tk, weight, root, bias)):
        # float64 throughout but for the weights' float32 rounding: 2^-24 relative per term, 1e-6 with room for the sums
        assert float((got - ref.double()).abs().max()) <= 1e-6 * float(ref.abs().max())


def test_no_dropout_and_no_window_is_the_parent_graph():
    ei, et, n, r = _graph(3)
    kept, hidden = R.kept_mask(ei.size(1), 0.0, seed=5, epoch=9, c0=77)
    assert kept.all() and not hidden.any()
    fw = O.bucket_ref(ei, et, n, r, transpose=False)
    bw = O.bucket_ref(ei, et, n, r, transpose=True)
    k = R.kept_counts(ei.numpy(), et.numpy(), kept, n, r)
    assert np.array_equal(np.maximum(k, 1).astype(np.float32), fw[3])            # the parent's cnt = max(1, segment size)
    w = R.weights(ei.numpy(), et.numpy(), kept, n, r)
    dst, rel = ei[1].numpy()[bw[2]], et.numpy()[bw[2]]
    want_wt = (np.float32(1.0) / fw[3][dst * r + rel]).astype(np.float32)          # the parent's w_t, same division
    assert np.array_equal(R.bucketed(w, bw[2]), want_wt)


@pytest.mark.parametrize("c0,batch,hidden_want", [(0, 0, 0), (0, 64, 64), (300, 128, 128), (650, 128, 50), (700, 64, 0)])
def test_the_window_hides_exactly_the_batch(c0, batch, hidden_want):
    e = 700
    order = np.random.default_rng(0).permutation(e)
    position = np.empty(e, dtype=np.int64)
    position[order] = np.arange(e)
    kept, hidden = R.kept_mask(e, 0.0, seed=1, epoch=1, c0=c0, batch=batch, position=position)
    assert int(hidden.sum()) == hidden_want and np.array_equal(kept, ~hidden)
    assert set(np.nonzero(hidden)[0].tolist()) == set(order[c0:c0 + batch].tolist())


KEPT_FRACTION_SEED = 20260101      # the band below holds for it (and for any seed with probability 1 - 6e-7)


def test_kept_fraction_on_200000_edges():
    e, p = 200_000, 0.4
    kept, _ = R.kept_mask(e, p, seed=KEPT_FRACTION_SEED, epoch=1, c0=0)
    q = 1.0 - R.threshold(p) / 2.0 ** 32              # the exact keep probability of the integer compare
    sd = math.sqrt(e * q * (1.0 - q))
    assert abs(q - 0.6) < 2.0 ** -32
    assert abs(int(kept.sum()) - 0.6 * e) <= 5.0 * sd, (int(kept.sum()), 0.6 * e, sd)
    # another cursor is another mask of the same fraction
    other, _ = R.kept_mask(e, p, seed=KEPT_FRACTION_SEED, epoch=1, c0=1024)
    assert abs(int(other.sum()) - 0.6 * e) <= 5.0 * sd and 0.4 * e < int((kept != other).sum()) < 0.56 * e


def test_threshold_is_the_integer_the_header_states():
    assert R.threshold(0.0) == 0 and R.threshold(0.5) == 1 << 31 and R.threshold(1.0 - 2.0 ** -53) == (1 << 32) - 1
    assert R.threshold(0.4) == int(np.floor(0.4 * 2.0 ** 32)) == 1717986918
    with pytest.raises(ValueError):
        R.threshold(1.0)


# ---------------------------------------------------------------------------------- trainer, models, command line
def test_cli_flags_default_off_and_reach_the_checkpoint_args():
    a = train.parse_args([])
    assert a.edge_dropout == 0.0 and a.hide_batch_edges is False
    b = train.parse_args(["--edge_dropout", "0.4", "--hide_batch_edges"])
    assert b.edge_dropout == 0.4 and b.hide_batch_edges is True     # save_checkpoint stores the namespace whole ("args")


@pytest.mark.parametrize("flags", [dict(edge_dropout=0.4), dict(hide_batch_edges=True), dict(edge_dropout=0.2, hide_batch_edges=True)])
def test_trainer_refuses_the_flags_on_the_cpu(tmp_path, flags):
    n, r = 50, 3
    gen = torch.Generator().manual_seed(0)
    data = {"edge_index": torch.randint(0, n, (2, 300), generator=gen), "edge_type": torch.randint(0, r, (300,), generator=gen),
            "num_nodes": n, "num_relations": r}
    args = train.parse_args([])
    args.output_dir, args.device = str(tmp_path), "cpu"
    for k, v in flags.items():
        setattr(args, k, v)
    model = train.create_model(n, r, args)
    with pytest.raises(ValueError, match="GPU only"):
        train.Trainer(model, data, data, data, torch.device("cpu"), args)


def test_trainer_refuses_a_probability_outside_the_half_open_interval(tmp_path):
    n, r = 50, 3
    data = {"edge_index": torch.zeros(2, 4, dtype=torch.int64), "edge_type": torch.zeros(4, dtype=torch.int64),
            "num_nodes": n, "num_relations": r}
    args = train.parse_args([])
    args.output_dir, args.edge_dropout = str(tmp_path), 1.0
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        train.Trainer(train.create_model(n, r, args), data, data, data, torch.device("cpu"), args)


def test_trainer_refuses_an_encoder_without_a_view(tmp_path):
    """the partitioned / replicated encoders of dist.py hold shard structures: refused by type, before any device work"""
    import torch.nn as nn
    n, r = 50, 3
    data = {"edge_index": torch.zeros(2, 4, dtype=torch.int64), "edge_type": torch.zeros(4, dtype=torch.int64),
            "num_nodes": n, "num_relations": r}
    args = train.parse_args([])
    args.output_dir, args.edge_dropout = str(tmp_path), 0.3
    model = train.create_model(n, r, args)
    model.encoder = nn.Identity()

    class _Cuda:                              # a device that says "cuda" without being one: the type check comes first
        type = "cuda"
    with pytest.raises(ValueError, match="dist.py"):
        train.Trainer(model, data, data, data, _Cuda(), args)
