"""GPU tier of the device bootstrap (``csrc/resample.hip``): the three entry points against the host restatement of
``include/rgcn_resample.h`` (``resample_reference.py``) - every integer EQUAL, the two doubles inside the bound the
header derives - at the sizes where the tile walk can go wrong (``T = RGCN_RESAMPLE_TILE``: one sample, a ragged
quad, one short of a tile, a tile, one more, several tiles and a ragged tail) and with tie groups laid across the tile
boundaries; then the callers: ``compare_methods(bootstrap=...)`` and the split by disease frequency."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import resample_reference as R
from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import _lib, bootstrap, ops, synth
from primekg_rgcn_linkprediction_amd import compare as C
from primekg_rgcn_linkprediction_amd import evaluate as E

pytestmark = pytest.mark.gpu

T = _lib.RESAMPLE_TILE
SEED = (0x1234ABCD << 32) | 0x0BADF00D          # a non-zero high word: both key words are used
REPS = 9                                        # replicate 0, two full groups of four and one of one
U53 = Fraction(1, 2 ** 53)


# ---------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("units", [1, 63, 64, 65, 1000])
def test_weights_equal_the_host_rule(units):
    dev = need_gpu()
    for reps in (0, 1, 4, 5, 9):
        got = ops.resample_weights(units, reps, SEED, device=dev).cpu().numpy()
        assert got.shape == (reps + 1, units) and got.dtype == np.uint8
        assert (got[0] == 1).all()
        for b in range(reps + 1):
            assert got[b].tolist() == R.weights(np.arange(units), b, SEED).tolist(), (units, reps, b)


# ---------------------------------------------------------------------------------- curves
def _check_counts(dev, scores, labels, units=None, threshold=0.5, reps=REPS, seed=SEED, dtype=torch.float32):
    """every replicate of one call against the reference on the same (rounded-to-dtype) scores"""
    scores_t = torch.as_tensor(np.asarray(scores, dtype=np.float64)).to(dtype)
    host_scores = scores_t.double().numpy()
    unit_t = None if units is None else torch.as_tensor(np.asarray(units), dtype=torch.int32).to(dev)
    got = ops.classification_counts(scores_t.to(dev), torch.as_tensor(np.asarray(labels)).to(dev), unit_t, reps, seed, threshold)
    n = len(host_scores)
    for f in got._fields:
        t = getattr(got, f)
        assert t.shape == (reps + 1,) and t.dtype == (torch.float64 if f == "ap" else torch.int64), f
    out = {f: getattr(got, f).cpu().tolist() for f in got._fields}
    ordered = R.sort_samples(host_scores, labels, units)
    for b in range(reps + 1):
        want = R.curves_sorted(*ordered, threshold, b, seed)
        for f in ("wp", "wn", "auc2", "tp", "fp"):
            assert out[f][b] == want[f], (f, b, out[f][b], want[f])
        err = abs(Fraction(out["ap"][b]) - want["ap"])
        assert err <= (n + 2) * U53, (b, float(err), float((n + 2) * U53))
    return got


def _descending(n, groups=()):
    """scores that fall with the position, with every ``(first, last)`` run of positions made equal; handed over in a
    shuffled order (the wrapper's sort has work to do)"""
    s = np.arange(n, 0, -1, dtype=np.float64) / 8192.0            # exact in float32, distinct, inside (0, 1) for n < 8192
    for first, last in groups:
        s[first:last + 1] = s[first]
    perm = np.random.RandomState(n).permutation(n)
    return s[perm]


@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 3 * T + 5])
def test_counts_at_every_size(n):
    dev = need_gpu()
    rng = np.random.RandomState(n)
    labels = (rng.rand(n) < 0.4).astype(np.int64)
    _check_counts(dev, np.round(rng.rand(n), 2), labels)                         # 101 values: ties everywhere
    _check_counts(dev, _descending(n), labels)                                   # all distinct
    _check_counts(dev, np.full(n, 0.25), labels)                                 # all equal: one group over every tile
    # shared units: positive i and negative i on one unit
    half = (n + 1) // 2
    units = np.r_[np.arange(half), np.arange(n - half)]
    _check_counts(dev, np.round(rng.rand(n), 1), np.r_[np.ones(half, np.int64), np.zeros(n - half, np.int64)], units)


LAYOUTS = {"across_a_boundary": (3 * T + 5, [(T - 2, T + 3)]),
           "three_whole_tiles_and_one_either_side": (4 * T + 3, [(T - 1, 4 * T)]),
           "ends_on_a_tile's_last_sample": (3 * T + 5, [(T - 5, T - 1), (2 * T - 1, 2 * T - 1), (3 * T - 2, 3 * T - 1)]),
           "starts_on_a_tile's_first_sample": (3 * T + 5, [(T, T + 1), (2 * T, 3 * T + 4)])}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_tie_groups_across_tiles(layout):
    dev = need_gpu()
    n, groups = LAYOUTS[layout]
    scores = _descending(n, groups)
    labels = (np.random.RandomState(7).rand(n) < 0.5).astype(np.int64)
    _check_counts(dev, scores, labels)
    # the threshold ON the tied score: the whole group is predicted positive
    first, last = groups[0]
    got = _check_counts(dev, scores, labels, threshold=float(np.sort(scores)[::-1][first]), reps=1)
    assert int(got.tp[0] + got.fp[0]) == last + 1


def test_degenerate_labels_and_thresholds():
    dev = need_gpu()
    n = T + 1
    rng = np.random.RandomState(3)
    scores = np.round(rng.rand(n), 2)
    for labels in (np.ones(n, np.int64), np.zeros(n, np.int64)):
        got = _check_counts(dev, scores, labels)
        assert got.auc2.tolist() == [0] * (REPS + 1) and got.ap.tolist() == [0.0] * (REPS + 1)
        assert bool(got.degenerate().all()) and bool(torch.isnan(got.auc_roc()).all()) and bool(torch.isnan(got.auc_pr()).all())
    labels = (rng.rand(n) < 0.5).astype(np.int64)
    below = _check_counts(dev, scores, labels, threshold=-1.0)
    assert torch.equal(below.tp, below.wp) and torch.equal(below.fp, below.wn)
    above = _check_counts(dev, scores, labels, threshold=2.0)
    assert above.tp.tolist() == [0] * (REPS + 1) and above.fp.tolist() == [0] * (REPS + 1)
    assert bool(torch.isnan(above.precision()).all()) and above.recall().tolist() == [0.0] * (REPS + 1)
    _check_counts(dev, scores, labels, threshold=0.5, dtype=torch.float64)
    # a replicate that leaves a class without weight: one positive, and seeds until its weight is 0 somewhere
    labels = np.zeros(5, np.int64)
    labels[2] = 1
    seed = next(s for s in range(100) if any(R.weight(2, b, s) == 0 for b in range(1, 5)))
    got = _check_counts(dev, [0.9, 0.8, 0.7, 0.6, 0.5], labels, reps=4, seed=seed)
    dead = [b for b in range(1, 5) if R.weight(2, b, seed) == 0]
    assert all(got.wp[b] == 0 and got.auc2[b] == 0 and got.ap[b] == 0.0 for b in dead) and got.wp[0] == 1


def test_non_finite_scores_count_with_their_neighbours():
    """+inf in front of every number, -inf behind, and NaN WITH -inf: a NaN never ranks above a number"""
    dev = need_gpu()
    n = T + 7
    rng = np.random.RandomState(11)
    scores = np.round(rng.randn(n), 1)
    scores[rng.permutation(n)[:40]] = np.repeat([np.inf, -np.inf, np.nan, np.nan], 10)
    labels = (rng.rand(n) < 0.5).astype(np.int64)
    got = _check_counts(dev, scores, labels, threshold=0.0)
    as_inf = np.where(np.isnan(scores), -np.inf, scores)
    same = ops.classification_counts(torch.as_tensor(as_inf, dtype=torch.float32).to(dev), torch.as_tensor(labels).to(dev), None,
                                     REPS, SEED, 0.0)
    assert all(torch.equal(a, b) for a, b in zip(got, same))
    # a NaN positive behind every number: the worst place a positive can have
    got = _check_counts(dev, [float("nan"), 0.1, 0.2, 0.3], [1, 0, 0, 0], reps=0)
    assert float(got.auc_roc()[0]) == 0.0


def test_replicate_zero_is_what_scikit_learn_reports():
    dev = need_gpu()
    n = 3 * T + 5
    rng = np.random.RandomState(5)
    scores = np.round(rng.rand(n), 2).astype(np.float32).astype(np.float64)
    labels = (rng.rand(n) < np.clip(scores, 0.1, 0.9)).astype(np.int64)
    want = E.ModelEvaluator.compute_classification_metrics(scores, labels)
    got = ops.classification_counts(torch.as_tensor(scores, dtype=torch.float32).to(dev), torch.as_tensor(labels).to(dev))
    mine = {"auc_roc": got.auc_roc(), "auc_pr": got.auc_pr(), "precision": got.precision(), "recall": got.recall(),
            "f1_score": got.f1()}
    for name, v in mine.items():
        assert v.shape == (1,) and abs(float(v[0]) - want[name]) <= 1e-12, (name, float(v[0]), want[name])
    assert abs(float(got.accuracy()[0]) - float(((scores >= 0.5) == (labels == 1)).mean())) <= 1e-12


def test_same_call_same_bytes_and_the_seed_moves_only_the_replicates():
    dev = need_gpu()
    n = 2 * T + 3
    rng = np.random.RandomState(9)
    scores = torch.as_tensor(np.round(rng.rand(n), 2), dtype=torch.float32).to(dev)
    labels = torch.as_tensor((rng.rand(n) < 0.5).astype(np.int64)).to(dev)
    ranks = torch.as_tensor(rng.randint(1, 500, n)).to(dev)
    a, b = (ops.classification_counts(scores, labels, None, REPS, SEED) for _ in range(2))
    other = ops.classification_counts(scores, labels, None, REPS, SEED + 1)
    for x, y, z in zip(a, b, other):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))
        assert torch.equal(x[:1].view(torch.int64), z[:1].view(torch.int64))
    assert not torch.equal(a.wp[1:], other.wp[1:]) and not torch.equal(a.auc2[1:], other.auc2[1:])
    ra, rb = (ops.rank_sums(ranks, None, (1, 10), REPS, SEED) for _ in range(2))
    ro = ops.rank_sums(ranks, None, (1, 10), REPS, SEED + 1)
    for x, y, z in zip(ra[:4], rb[:4], ro[:4]):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64)) and torch.equal(x[:1].view(torch.int64), z[:1].view(torch.int64))
    assert not torch.equal(ra.w_sum[1:], ro.w_sum[1:])


# ---------------------------------------------------------------------------------- ranks
@pytest.mark.parametrize("m", [1, T + 1, 2 * T + 3])
@pytest.mark.parametrize("nk", [1, 8])
def test_rank_sums_against_the_reference(m, nk):
    dev = need_gpu()
    rng = np.random.RandomState(m + nk)
    k_values = [1, 3, 5, 10, 20, 50, 100, 1000][:nk] if nk > 1 else [10]
    ranks = rng.randint(1, 30000, m)
    ranks[rng.permutation(m)[:max(m // 4, 1)]] = 1                       # ranks of 1, and values above every k
    b = (m + 1) // 2
    units = np.arange(m) % b                                             # both sides: query i belongs to triple i mod b
    got = ops.rank_sums(torch.as_tensor(ranks).to(dev), torch.as_tensor(units, dtype=torch.int32).to(dev), k_values, REPS, SEED)
    assert got.hit_sums.shape == (REPS + 1, nk) and got.rr_sum.dtype == torch.float64
    w_sum, rank_sum, hits, rr = got.w_sum.tolist(), got.rank_sum.tolist(), got.hit_sums.tolist(), got.rr_sum.tolist()
    for r in range(REPS + 1):
        want = R.rank_sums(ranks, units, k_values, r, SEED)
        assert (w_sum[r], rank_sum[r], hits[r]) == (want["w_sum"], want["rank_sum"], want["hits"]), r
        assert abs(Fraction(rr[r]) - want["rr_sum"]) <= (m + 2) * U53 * want["rr_sum"], r
    assert w_sum[0] == m and float(got.hits(k_values[0])[0]) == float(np.mean(ranks <= k_values[0]))
    assert float(got.mean_rank()[0]) == float(ranks.sum()) / m


# ---------------------------------------------------------------------------------- callers
@pytest.fixture(scope="module")
def synthetic():
    from primekg_rgcn_linkprediction_amd import train as TR
    tr, va, full, te = TR.synthetic_data(num_edges=20000, seed=4)
    return tr, te, full, synth.primekg_like_node_classes()


def test_compare_methods_with_a_bootstrap(synthetic, monkeypatch):
    dev = need_gpu()
    tr, te, full, classes = synthetic
    kw = dict(methods=("random", "degree"), both_sides=True, seed=3, drug_class=1, disease_class=0)
    plain = C.compare_methods(tr, te, full, dev, None, classes, **kw)
    assert set(plain) == {"protocol", "methods"} and "bootstrap" not in plain["protocol"]
    assert all(set(m) == {"ranking", "classification", "fit_seconds"} for m in plain["methods"].values())
    assert "±" not in C.table_markdown(plain)
    seen = []                                         # what the two device calls were handed, read back from the device
    counts, sums = ops.classification_counts, ops.rank_sums
    monkeypatch.setattr(ops, "classification_counts", lambda s, y, u, *a: (seen.append(("c", s.cpu(), y.cpu(), u.cpu())), counts(s, y, u, *a))[1])
    monkeypatch.setattr(ops, "rank_sums", lambda r, u, *a: (seen.append(("r", r.cpu(), u.cpu())), sums(r, u, *a))[1])
    result = C.compare_methods(tr, te, full, dev, None, classes, bootstrap=8, bootstrap_seed=SEED, **kw)
    b = te["edge_index"].size(1)
    assert [s[0] for s in seen] == ["c", "r", "c", "r"]
    assert result["protocol"]["bootstrap"]["replicates"] == 8 and set(result) == {"protocol", "methods", "significance"}
    for name, m in result["methods"].items():
        assert {k: v for k, v in m.items() if k != "bootstrap"}.keys() == plain["methods"][name].keys()
        assert m["ranking"] == plain["methods"][name]["ranking"] and m["classification"] == plain["methods"][name]["classification"]
    for i, name in enumerate(("random", "degree")):
        (_, scores, labels, unit), (_, ranks, rank_unit) = seen[2 * i], seen[2 * i + 1]
        assert unit.tolist() == list(range(b)) * 2 and rank_unit.tolist() == list(range(b)) * 2 and ranks.numel() == 2 * b
        boot = result["methods"][name]["bootstrap"]
        assert (boot["replicates"], boot["seed"]) == (8, SEED) and len(boot["weight_sums"]) == 9
        values = boot["replicate_values"]
        ordered = R.sort_samples(scores.numpy(), labels.numpy(), unit.numpy())
        for r in range(9):
            c = R.curves_sorted(*ordered, 0.5, r, SEED)
            q = R.rank_sums(ranks.numpy(), rank_unit.numpy(), C.K_VALUES, r, SEED)
            assert values["auc_roc"][r] == c["auc2"] / (2 * c["wp"] * c["wn"])
            assert abs(Fraction(values["auc_pr"][r]) - c["ap"]) <= (2 * b + 2) * U53
            assert values["f1_score"][r] == 2 * c["tp"] / (c["tp"] + c["fp"] + c["wp"])
            assert values["mean_rank"][r] == q["rank_sum"] / q["w_sum"] and boot["weight_sums"][r] == q["w_sum"]
            assert [values[f"hits@{k}"][r] for k in C.K_VALUES] == [h / q["w_sum"] for h in q["hits"]]
            assert abs(Fraction(values["mrr"][r]) - q["rr_sum"] / q["w_sum"]) <= (2 * b + 4) * U53 * q["rr_sum"] / q["w_sum"]
        point = result["methods"][name]
        assert abs(boot["auc_roc"]["estimate"] - point["classification"]["auc_roc"]) <= 1e-12
        assert abs(boot["mrr"]["estimate"] - point["ranking"]["mrr"]) <= 1e-12 and boot["degenerate_replicates"] == 0
        assert boot["mrr"] == bootstrap.interval(np.array(values["mrr"]))
    ra, de = (result["methods"][n]["bootstrap"] for n in ("random", "degree"))
    assert ra["weight_sums"] == de["weight_sums"] and ra["weight_sums"][0] == 2 * b and len(set(ra["weight_sums"])) > 1
    assert set(result["significance"]) == {"auc_roc", "auc_pr", "mrr", "hits@10"}
    for metric, pairs in result["significance"].items():
        assert list(pairs) == ["random vs degree"] and 0 < pairs["random vs degree"]["p_value"] <= 1
        assert pairs["random vs degree"] == bootstrap.paired_difference(np.array(ra["replicate_values"][metric], dtype=float),
                                                                        np.array(de["replicate_values"][metric], dtype=float))
    assert "±" in C.table_markdown(result) and "| mrr | random vs degree |" in C.table_markdown(result)


def test_evaluator_bootstrap_block(synthetic):
    """``ModelEvaluator.bootstrap`` after ``evaluate``: the same scores, the units of the batched layout (three batches,
    two corruptions a triple), the estimates of ``evaluate`` and the restatement's replicate values"""
    dev = need_gpu()
    from primekg_rgcn_linkprediction_amd import DrugDiseaseModel
    tr, te, full, classes = synthetic
    torch.manual_seed(0)
    ev = E.ModelEvaluator(DrugDiseaseModel(full["num_nodes"], 3, 64, 128), te, full, dev, batch_size=64)
    b = ev.num_test_edges
    assert 2 * 64 < b <= 3 * 64
    metrics = ev.evaluate(num_neg_samples=2, k_values=(10, 50), both_sides=True)
    scores, labels = ev.scores.copy(), ev.labels.copy()
    boot = ev.bootstrap(8, SEED, both_sides=True, num_neg_samples=2, k_values=(10, 50))
    assert np.array_equal(ev.scores, scores) and set(metrics) == {"classification", "ranking", "test_edges", "num_nodes",
                                                                 "ranking_filtered"}
    units = ev._sample_units(2).cpu().numpy()
    want_units = np.concatenate([np.r_[np.arange(lo, min(lo + 64, b)), np.repeat(np.arange(lo, min(lo + 64, b)), 2)]
                                 for lo in range(0, b, 64)])
    assert units.tolist() == want_units.tolist() and units.size == scores.size == 3 * b
    assert {"auc_roc", "auc_pr", "f1_score", "mrr", "mean_rank", "hits@10", "hits@50", "replicates", "seed",
            "degenerate_replicates", "protocol"} <= set(boot)
    assert (boot["replicates"], boot["seed"], boot["degenerate_replicates"]) == (8, SEED, 0)
    assert boot["weight_sums"][0] == 2 * b and boot["protocol"]["sides"] == "both"
    for name in ("auc_roc", "auc_pr", "f1_score"):
        assert abs(boot[name]["estimate"] - metrics["classification"][name]) <= 1e-12, name
    for name in ("mrr", "mean_rank", "hits@10", "hits@50"):
        assert abs(boot[name]["estimate"] - metrics["ranking_filtered"][name]) <= 1e-12 * max(1, metrics["ranking_filtered"][name])
        lo, hi = boot[name]["ci95"]
        assert lo <= hi and (boot[name]["se"] > 0 or name.startswith("hits"))     # an untrained model may hit nothing
    ordered = R.sort_samples(scores.astype(np.float64), labels, units)
    for r in range(9):
        c = R.curves_sorted(*ordered, 0.5, r, SEED)
        assert boot["replicate_values"]["auc_roc"][r] == c["auc2"] / (2 * c["wp"] * c["wn"])
        assert c["wp"] * 2 == c["wn"]                                  # a triple's two corruptions carry its weight


@pytest.mark.parametrize("test_set", ["held_out", "every_relation"])
def test_by_frequency_splits_the_triples_with_a_disease_end(synthetic, test_set):
    """``held_out``: the synthetic split's own test triples - drug-gene pairs, none has a disease end, every stratum is
    empty and says so; ``every_relation``: every 211th column of the full graph, so triples of all three relations"""
    dev = need_gpu()
    tr, te, full, classes = synthetic
    if test_set == "every_relation":
        te = {"edge_index": full["edge_index"][:, ::211].contiguous(), "edge_type": full["edge_type"][::211].contiguous()}
    with pytest.raises(ValueError, match="by_frequency"):
        C.compare_methods(tr, te, full, dev, None, None, methods=("random",), by_frequency=True)
    result = C.compare_methods(tr, te, full, dev, None, classes, methods=("random", "degree"), seed=3, drug_class=1,
                               disease_class=0, by_frequency=True, bootstrap=4)
    cls = classes.numpy()
    head, tail = te["edge_index"].numpy()
    degree = np.bincount(tr["edge_index"].numpy().reshape(-1), minlength=cls.size)
    q1, q2 = np.percentile(degree[(cls == 0) & (degree > 0)], [33, 67])
    block = result["by_frequency"]
    assert block["boundaries"] == {"q33": float(q1), "q67": float(q2)}
    end = np.where(cls[tail] == 0, tail, head)
    has = cls[end] == 0
    want = {"rare": has & (degree[end] <= q1), "medium": has & (degree[end] > q1) & (degree[end] <= q2),
            "common": has & (degree[end] > q2)}
    assert block["triples"] == {k: int(v.sum()) for k, v in want.items()} and sum(block["triples"].values()) == int(has.sum())
    assert (int(has.sum()) == 0) == (test_set == "held_out") and (test_set == "held_out" or 0 < int(has.sum()) < has.size)
    strata = C.frequency_strata(tr["edge_index"].to(dev), te["edge_index"][0].to(dev), te["edge_index"][1].to(dev),
                                classes.to(dev), 0)
    masks = {k: strata[k].cpu().numpy() for k in C.STRATA}
    assert all((masks[k] == want[k]).all() for k in C.STRATA)
    assert (sum(m.astype(int) for m in masks.values()) == has.astype(int)).all()          # a partition of the triples with one
    for name in ("random", "degree"):
        per = block["methods"][name]
        assert set(per) == set(C.STRATA)
        for k in C.STRATA:
            assert per[k]["triples"] == block["triples"][k]
            if per[k]["triples"]:
                assert set(per[k]) == {"triples", "ranking", "classification", "bootstrap"}
                assert per[k]["bootstrap"]["weight_sums"][0] == per[k]["triples"] and per[k]["bootstrap"]["replicates"] == 4
                assert set(per[k]["ranking"]) == set(C.ranking_metrics(torch.tensor([1])))
