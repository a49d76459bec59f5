"""CPU tier of twin-aware edge dropout (``RGCN_EDGE_DROPOUT_HIDE_TWINS`` / ``RGCN_EDGE_DROPOUT_PAIRED`` of
``include/rgcn_edge_dropout.h``; ``ops.EdgeDropout.draw(hide_twins=, paired=)``; ``train.py --hide_reverse_edges
--paired_edge_dropout``): the host restatement of the twin contract and of the two draw rules
(``edge_dropout_twins_reference.py``), the argument checks that run before any launch, the trainer's refusals, the two
parser flags and the header's macros."""
import math
import re

import numpy as np
import pytest
import torch

import c_surface as S
import edge_dropout_reference as R
import edge_dropout_twins_reference as TW
from primekg_rgcn_linkprediction_amd import _lib, ops, train

SEED = 20260101                      # the seed of tests/test_edge_dropout_host.py's band


# ---------------------------------------------------------------------------------- the header
def test_header_names_both_option_bits_and_the_abi_version_stays():
    header = S.header_text("rgcn_edge_dropout.h")
    bits = {name: int(shift) for name, shift in re.findall(r"#define (RGCN_EDGE_DROPOUT_[A-Z_]+)\s+\(1LL << (\d+)\)", header)}
    assert bits == {"RGCN_EDGE_DROPOUT_HIDE_TWINS": 62, "RGCN_EDGE_DROPOUT_PAIRED": 61}
    assert (1 << 62, 1 << 61) == (TW.HIDE_TWINS, TW.PAIRED) == (_lib.EDGE_DROPOUT_HIDE_TWINS, _lib.EDGE_DROPOUT_PAIRED)
    assert "#define RGCN_ABI_VERSION 38\n" in S.header_text("rgcn_hip.h")
    # the contract is stated where the draw's is: the words the restatement is written from
    for phrase in ("twin[F[j]] = B[j]", "SURPLUS", "involution", "in_window(twin[e])", "min(e, twin[e])"):
        assert phrase in header, phrase


# ---------------------------------------------------------------------------------- the twin contract
def _columns(triples):
    src, rel, dst = (np.array(v, dtype=np.int64) for v in zip(*triples))
    return np.stack([src, dst]), rel


def test_reversed_triple_with_equal_relation_self_loops_and_unmatched_columns():
    #            0          1          2          3          4          5          6          7
    triples = [(1, 0, 2), (3, 1, 3), (2, 0, 1), (4, 2, 5), (2, 1, 1), (1, 0, 1), (5, 0, 4), (6, 1, 7)]
    ei, et = _columns(triples)
    #  0 <-> 2 (1, 0, 2) / (2, 0, 1); 3 and 6 differ in the relation; 4 has the relation of no (1, 1, 2); 1 and 5 are loops
    assert TW.twins(ei, et).tolist() == [2, -1, 0, -1, -1, -1, -1, -1]
    assert TW.twins(ei, et).dtype == np.int32


def test_decoys_with_another_relation_are_not_twins():
    ei, et = _columns([(7, 0, 9), (9, 1, 7), (9, 0, 7), (7, 1, 9)])
    assert TW.twins(ei, et).tolist() == [2, 3, 0, 1]
    ei, et = _columns([(7, 0, 9), (9, 1, 7)])
    assert TW.twins(ei, et).tolist() == [-1, -1]


def test_two_copies_against_three_pair_in_column_order():
    #            0          1          2          3          4          5
    triples = [(8, 2, 3), (3, 2, 8), (0, 0, 0), (3, 2, 8), (8, 2, 3), (8, 2, 3)]
    ei, et = _columns(triples)
    # B = (3, 2, 8): columns 1, 3; F' = (8, 2, 3): columns 0, 4, 5 - the first two of each pair, column 5 is surplus
    assert TW.twins(ei, et).tolist() == [1, 0, -1, 4, 3, -1]


def _random_graph(seed, n=23, r=3, e=1500):
    """dense enough that triples repeat with unequal multiplicities on the two sides, with self loops"""
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, n, (2, e))
    et = rng.integers(0, r, e)
    ei[1, :40] = ei[0, :40]
    return ei, et


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_twin_is_an_involution_between_reversed_triples_and_counts_min_of_both_sides(seed):
    ei, et = _random_graph(seed)
    twin = TW.twins(ei, et)
    has = np.nonzero(twin >= 0)[0]
    assert 0 < has.size < twin.size
    t = twin[has]
    assert np.array_equal(twin[t], has) and bool((t != has).all())                      # an involution without fixed points
    assert np.array_equal(ei[0, t], ei[1, has]) and np.array_equal(ei[1, t], ei[0, has]) and np.array_equal(et[t], et[has])
    assert bool((ei[0, has] != ei[1, has]).all())                                      # no self loop has one
    # per ordered triple: min(|F|, |B|) columns have a twin, and they are the FIRST ones, paired in order
    cols = {}
    for e, key in enumerate(zip(ei[0].tolist(), et.tolist(), ei[1].tolist())):
        cols.setdefault(key, []).append(e)
    surplus = 0
    for (a, r, b), f in cols.items():
        back = cols.get((b, r, a), []) if a != b else []
        m = min(len(f), len(back))
        assert twin[f[:m]].tolist() == back[:m] and bool((twin[f[m:]] == -1).all())
        surplus += len(f) - m if back else 0
    assert surplus > 0                                                                 # the case is in the graph


# ---------------------------------------------------------------------------------- the two draw rules
def _window(e, seed=3):
    order = np.random.default_rng(seed).permutation(e)
    position = np.empty(e, dtype=np.int64)
    position[order] = np.arange(e)
    return order, position


def test_neither_option_is_the_plain_restatement():
    ei, et = _random_graph(4)
    e = ei.shape[1]
    twin = TW.twins(ei, et)
    _, position = _window(e)
    for p, c0, batch, pos in ((0.4, 0, 0, None), (0.4, 100, 64, position), (0.0, e - 10, 64, position)):
        want = R.kept_mask(e, p, SEED, 2, c0, batch, pos)
        got = TW.kept_mask(e, twin, p, SEED, 2, c0, batch, pos)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_hide_twins_hides_the_window_and_the_twins_of_its_columns_and_nothing_else():
    ei, et = _random_graph(5)
    e = ei.shape[1]
    twin = TW.twins(ei, et)
    order, position = _window(e)
    for c0, batch in ((0, 64), (700, 128), (e - 20, 64)):
        kept, hidden = TW.kept_mask(e, twin, 0.0, SEED, 1, c0, batch, position, hide_twins=True)
        cols = order[c0:c0 + batch]
        want = set(cols.tolist()) | {int(t) for t in twin[cols] if t >= 0}
        assert set(np.nonzero(hidden)[0].tolist()) == want and len(want) > len(cols)
        assert np.array_equal(kept, ~hidden)
    # without a position nothing is hidden, whatever the bit says
    assert not TW.hidden_mask(e, twin, 0, 64, None, hide_twins=True).any()


def test_a_paired_draw_marks_both_members_of_every_pair_alike():
    ei, et = _random_graph(6)
    e = ei.shape[1]
    twin = TW.twins(ei, et)
    order, position = _window(e)
    has = np.nonzero(twin >= 0)[0]
    plain, _ = TW.kept_mask(e, twin, 0.4, SEED, 1, 512)
    assert bool((plain[has] != plain[twin[has]]).any())                                # what the option is for
    for hide_twins in (False, True):
        kept, hidden = TW.kept_mask(e, twin, 0.4, SEED, 1, 512, 128, position, hide_twins=hide_twins, paired=True)
        dropped = TW.words(e, twin, SEED, 1, 512, paired=True) < R.threshold(0.4)
        assert np.array_equal(dropped[has], dropped[twin[has]])
        assert np.array_equal(dropped[twin < 0], (R.words(e, SEED, 1, 512) < R.threshold(0.4))[twin < 0])   # the others: their own word
        if hide_twins:                                                                 # then the whole mark agrees, not only the drop
            assert np.array_equal(kept[has], kept[twin[has]]) and np.array_equal(hidden[has], hidden[twin[has]])
    # the shared word is the lower column's
    w, w_plain = TW.words(e, twin, SEED, 1, 512, paired=True), R.words(e, SEED, 1, 512)
    assert np.array_equal(w[has], w_plain[np.minimum(has, twin[has])])


def test_paired_kept_fraction_on_200000_columns_that_all_have_a_twin():
    """the band of tests/test_edge_dropout_host.py::test_kept_fraction_on_200000_edges - five binomial standard deviations
    - with the deviation counted over the 100,000 PAIRS: the two members of a pair share one word, so the kept count is
    twice a binomial over the pairs, not a binomial over the columns"""
    pairs, p, n = 100_000, 0.4, 5000
    rng = np.random.default_rng(7)
    a = rng.integers(0, n, pairs)
    b = (a + rng.integers(1, n, pairs)) % n                                            # a != b
    rel = rng.integers(0, 4, pairs)
    ei = np.empty((2, 2 * pairs), dtype=np.int64)
    ei[0, 0::2], ei[1, 0::2], ei[0, 1::2], ei[1, 1::2] = a, b, b, a                      # every pair: two adjacent columns
    et = np.repeat(rel, 2)
    e = 2 * pairs
    twin = TW.twins(ei, et)
    assert bool((twin >= 0).all()) and np.array_equal(twin[twin], np.arange(e))
    kept, _ = TW.kept_mask(e, twin, p, SEED, 1, 0, paired=True)
    assert np.array_equal(kept, kept[twin])
    q = 1.0 - R.threshold(p) / 2.0 ** 32
    sd_pairs = math.sqrt(pairs * q * (1.0 - q))
    kept_pairs = int(kept.sum()) // 2
    assert int(kept.sum()) == 2 * kept_pairs
    assert abs(kept_pairs - q * pairs) <= 5.0 * sd_pairs, (kept_pairs, q * pairs, sd_pairs)


# ---------------------------------------------------------------------------------- ops: checks before any launch
class _Alive:
    alive, num_edges, device = True, 100, torch.device("cpu")


def _bare_dropout():
    """an ``ops.EdgeDropout`` around a fake handle: ``draw`` checks its arguments before it loads the library"""
    ed = ops.EdgeDropout.__new__(ops.EdgeDropout)
    ed._handle, ed.graph, ed.device = S.FAKE_BASE, _Alive(), torch.device("cpu")
    return ed


def test_draw_refuses_a_batch_that_reaches_the_option_bits_and_twins_without_a_position():
    ed = _bare_dropout()
    rng = torch.zeros(2, dtype=torch.int64)
    try:
        for batch in (1 << 61, 1 << 62, (1 << 61) | 5, -1):
            with pytest.raises(ValueError, match="batch"):
                ed.draw(0.4, rng, batch=batch)
        with pytest.raises(ValueError, match="position"):
            ed.draw(0.4, rng, batch=8, hide_twins=True)
        with pytest.raises(ValueError, match="position"):
            ed.draw(0.4, rng, batch=8, hide_twins=True, paired=True)
    finally:
        ed._handle = None                                # nothing to destroy


# ---------------------------------------------------------------------------------- trainer and command line
def test_cli_flags_default_off_and_reach_the_checkpoint_args():
    a = train.parse_args([])
    assert a.hide_reverse_edges is False and a.paired_edge_dropout is False
    b = train.parse_args(["--edge_dropout", "0.4", "--hide_batch_edges", "--hide_reverse_edges", "--paired_edge_dropout"])
    assert b.hide_reverse_edges is True and b.paired_edge_dropout is True and b.hide_batch_edges is True   # "args" of a checkpoint


@pytest.mark.parametrize("flags,match", [(dict(hide_reverse_edges=True), "--hide_batch_edges"),
                                         (dict(hide_reverse_edges=True, edge_dropout=0.4), "--hide_batch_edges"),
                                         (dict(paired_edge_dropout=True), "--edge_dropout"),
                                         (dict(paired_edge_dropout=True, hide_batch_edges=True), "--edge_dropout")])
def test_trainer_refuses_a_flag_without_the_one_it_builds_on(tmp_path, flags, match):
    n, r = 50, 3
    data = {"edge_index": torch.zeros(2, 4, dtype=torch.int64), "edge_type": torch.zeros(4, dtype=torch.int64),
            "num_nodes": n, "num_relations": r}
    args = train.parse_args([])
    args.output_dir = str(tmp_path)
    for k, v in flags.items():
        setattr(args, k, v)
    with pytest.raises(ValueError, match=match):
        train.Trainer(train.create_model(n, r, args), data, data, data, torch.device("cpu"), args)


def test_trainer_with_all_four_flags_is_refused_on_the_cpu_like_its_siblings(tmp_path):
    n, r = 50, 3
    data = {"edge_index": torch.zeros(2, 4, dtype=torch.int64), "edge_type": torch.zeros(4, dtype=torch.int64),
            "num_nodes": n, "num_relations": r}
    args = train.parse_args(["--edge_dropout", "0.4", "--hide_batch_edges", "--hide_reverse_edges", "--paired_edge_dropout"])
    args.output_dir = str(tmp_path)
    with pytest.raises(ValueError, match="GPU only"):
        train.Trainer(train.create_model(n, r, args), data, data, data, torch.device("cpu"), args)
