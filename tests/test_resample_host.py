"""CPU tier of the device bootstrap (``csrc/resample.hip``, ``include/rgcn_resample.h``, ``bootstrap.py``): the host
restatement of the contract (``resample_reference.py``) against scikit-learn and against the definition of its own
constants, the interval and p-value arithmetic on hand-made arrays, the C surface (prototypes, every refusal that comes
before a launch) and the command lines' new flags."""
import decimal
import os
import re

import numpy as np
import pytest
import torch

import c_surface as S
import resample_reference as R
from c_surface import STREAM, T4, T8, T16
from conftest import ROOT
from primekg_rgcn_linkprediction_amd import _lib, bootstrap, compare, evaluate, ops



# ---------------------------------------------------------------------------------- the rule
def test_host_philox_reproduces_the_published_vectors_and_its_array_form():
    f = R.M32
    assert R.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert R.philox4x32_10((f, f, f, f), (f, f)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    seed = (0x9E3779B9 << 32) | 0x7F4A7C15
    units = np.array([0, 1, 63, 64, 65, 1000, 2 ** 31 - 1])
    for b in (0, 1, 2, 3, 4, 5, 8, 9, 65535):
        assert R.weights(units, b, seed).tolist() == [R.weight(int(u), b, seed) for u in units], b
    assert R.weights(units, 0, seed).tolist() == [1] * len(units)
    # replicates 1 .. 4 are the four words of ONE call, replicate 5 starts the next
    c = R.philox4x32_10((65, 0, R.STREAM, 0), (seed & f, seed >> 32))
    assert [R.weight(65, b, seed) for b in (1, 2, 3, 4)] == [R.weight_of_word(w) for w in c]
    c = R.philox4x32_10((65, 1, R.STREAM, 0), (seed & f, seed >> 32))
    assert R.weight(65, 5, seed) == R.weight_of_word(c[0])


def test_thresholds_are_the_poisson_cdf_and_the_header_holds_them():
    decimal.getcontext().prec = 60
    e_inv, term, cdf, want = decimal.Decimal(-1).exp(), decimal.Decimal(1), decimal.Decimal(0), []
    for k in range(13):
        term = term / k if k else term
        cdf += e_inv * term
        want.append(int((cdf * 2 ** 32).to_integral_value(rounding=decimal.ROUND_FLOOR)))
    assert tuple(want) == R.THRESHOLDS and want[-1] == 2 ** 32 - 1 and len(set(want)) == 13
    header = open(os.path.join(ROOT, "include", "rgcn_resample.h")).read()
    body = re.search(r"#define RGCN_RESAMPLE_THRESHOLDS\s*\\\s*\{(.*?)\}", header, flags=re.S).group(1)
    assert tuple(int(x) for x in re.findall(r"(\d+)u", body)) == R.THRESHOLDS
    assert f"#define RGCN_RESAMPLE_STREAM 0x{R.STREAM:08X}u" in header
    assert f"#define RGCN_RESAMPLE_TILE {_lib.RESAMPLE_TILE} " in header
    assert f"#define RGCN_RESAMPLE_MAX_SAMPLES {_lib.RESAMPLE_MAX_SAMPLES} " in header and _lib.RESAMPLE_MAX_SAMPLES == 2 ** 28
    assert f"#define RGCN_RESAMPLE_MAX_REPLICATES {_lib.RESAMPLE_MAX_REPLICATES}\n" in header
    assert f"#define RGCN_RESAMPLE_MAX_K {_lib.RESAMPLE_MAX_K} " in header
    assert [R.weight_of_word(w) for w in (0, want[0] - 1, want[0], want[1], 2 ** 32 - 2, 2 ** 32 - 1)] == [0, 0, 1, 2, 12, 13]


def test_the_mean_weight_is_one():
    """2^20 draws of a unit-variance variable: the mean's standard error is 2^-10, and five of them are allowed"""
    w = R.weights(np.arange(2 ** 20), 1, 12345)
    assert abs(w.mean() - 1.0) <= 5 / 1024
    assert w.min() == 0 and 5 <= w.max() <= 13


# ---------------------------------------------------------------------------------- the restatement against scikit-learn
def test_the_restatement_equals_scikit_learn_under_integer_weights():
    from sklearn.metrics import average_precision_score, roc_auc_score
    rng = np.random.RandomState(7)
    worst, done = 0.0, 0
    while done < 200:
        n = int(rng.randint(2, 401))
        scores = np.round(rng.rand(n), int(rng.randint(0, 3)))
        labels = (rng.rand(n) < rng.rand()).astype(np.int64)
        seed, b = int(rng.randint(0, 2 ** 31)), int(rng.randint(1, 10))
        w = R.weights(np.arange(n), b, seed)
        if (w * labels).sum() == 0 or (w * (1 - labels)).sum() == 0:
            continue
        got = R.curves(scores, labels, None, 0.5, b, seed)
        assert got["wp"] == int((w * labels).sum()) and got["wn"] == int((w * (1 - labels)).sum())
        auc = got["auc2"] / (2 * got["wp"] * got["wn"])
        worst = max(worst, abs(auc - roc_auc_score(labels, scores, sample_weight=w)),
                    abs(float(got["ap"]) - average_precision_score(labels, scores, sample_weight=w)))
        pred = scores >= 0.5
        assert got["tp"] == int((w * labels * pred).sum()) and got["fp"] == int((w * (1 - labels) * pred).sum())
        done += 1
    assert worst <= 1e-12, worst


def test_rank_sums_restated():
    got = R.rank_sums([1, 2, 10, 51, 4], [0, 1, 2, 0, 1], (1, 5, 10), 0, 3)
    assert got["w_sum"] == 5 and got["rank_sum"] == 68 and got["hits"] == [1, 3, 4]
    assert float(got["rr_sum"]) == pytest.approx(1 + 1 / 2 + 1 / 10 + 1 / 51 + 1 / 4)
    w = R.weights([0, 1, 2, 0, 1], 3, 3).tolist()
    assert w[0] == w[3] and w[1] == w[4]                             # a unit's queries share its weight
    assert R.rank_sums([1, 2, 10, 51, 4], [0, 1, 2, 0, 1], (5,), 3, 3)["hits"] == [w[0] + w[1] + w[4]]


# ---------------------------------------------------------------------------------- intervals and p-values
def test_interval_and_paired_p_value_on_hand_made_arrays():
    a = np.array([0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.3, 1.4])     # a point estimate and nine replicates
    zero = np.zeros(10)
    i = bootstrap.interval(a)
    assert i["estimate"] == 0.5 and i["se"] == pytest.approx(np.std(a[1:], ddof=1))
    assert i["ci95"] == [pytest.approx(0.6 + 0.8 * 0.025), pytest.approx(1.4 - 0.8 * 0.025)]
    # every difference positive: #{d <= 0} = 0, #{d >= 0} = 9 -> 2 min(1 / 10, 10 / 10)
    d = bootstrap.paired_difference(a, zero)
    assert d["p_value"] == pytest.approx(0.2) and d["replicates"] == 9 and d["difference"] == 0.5
    assert d["mean_difference"] == pytest.approx(1.0) and d["ci95"][0] > 0
    assert bootstrap.paired_difference(zero, a)["p_value"] == pytest.approx(0.2)
    # every difference zero: both counts are 9 -> min(1, 2 * 10 / 10)
    same = bootstrap.paired_difference(a, a)
    assert same["p_value"] == 1.0 and same["mean_difference"] == 0.0 and same["ci95"] == [0.0, 0.0]
    # mixed: d = -1, -1, 1, 1, 1, 1, 1, 1, 0 -> #{d <= 0} = 3, #{d >= 0} = 7 -> 2 * 4 / 10
    b = a.copy()
    b[1:] += np.array([1, 1, -1, -1, -1, -1, -1, -1, 0.0])
    assert bootstrap.paired_difference(a, b)["p_value"] == pytest.approx(0.8)
    # a replicate in which either method is undefined is dropped from both: three left, all positive -> 2 * 1 / 4
    c = a.copy()
    c[[2, 3, 4]] = np.nan
    z = zero.copy()
    z[[5, 6, 7]] = np.nan
    d = bootstrap.paired_difference(c, z)
    assert d["replicates"] == 3 and d["p_value"] == pytest.approx(0.5)
    assert bootstrap.interval(c)["se"] == pytest.approx(np.std(a[[1, 5, 6, 7, 8, 9]], ddof=1))
    none = bootstrap.paired_difference(np.array([0.5]), np.array([0.25]))
    assert none["p_value"] is None and none["difference"] == 0.25 and bootstrap.interval(np.array([0.5]))["se"] is None
    sig = bootstrap.significance({"x": {"mrr": a, "auc_roc": a}, "y": {"mrr": zero, "auc_roc": a}, "z": {"mrr": a, "auc_roc": zero}})
    assert list(sig) == ["auc_roc", "mrr"] and list(sig["mrr"]) == ["x vs y", "x vs z", "y vs z"]
    assert sig["mrr"]["x vs y"]["p_value"] == pytest.approx(0.2) and sig["mrr"]["x vs z"]["p_value"] == 1.0


def test_units_follow_the_sampler_layout():
    assert bootstrap.triple_units(3, 3, "cpu").tolist() == [0, 1, 2]
    assert bootstrap.triple_units(3, 6, "cpu").tolist() == [0, 1, 2, 0, 1, 2]
    assert bootstrap.triple_units(3, 9, "cpu").tolist() == [0, 1, 2, 0, 0, 1, 1, 2, 2]
    assert bootstrap.query_units(3, 6, "cpu").tolist() == [0, 1, 2, 0, 1, 2] and bootstrap.query_units(3, 3, "cpu").dtype == torch.int32


# ---------------------------------------------------------------------------------- C surface
def test_header_table_and_library_agree():
    """names, parameters, return types and exports: test_c_surface.py, for every header"""
    makefile = open(os.path.join(ROOT, "primekg_rgcn_linkprediction_amd", "csrc", "Makefile")).read()
    assert " resample.hip" in makefile


# argument sets at the smallest legal sizes, in the notation of c_surface.py
CURVES = [T4, T16, T4, 1, 1, 1, 1, 0, T8, T8, T8, T8, T8, T8, STREAM]
RANKS = [T8, T4, 1, T4, 1, 1, 1, 0, T8, T8, T8, T8, STREAM]
ALIGNMENT_CASES = {"rgcn_resample_curves": [CURVES], "rgcn_resample_ranks": [RANKS]}


def _values(args, shift_at=None, shift=0, **sizes):
    args = list(args)
    for pos, v in sizes.items():
        args[int(pos[1:])] = v
    return S.build(args, (shift_at, None), shift)[0]


@pytest.mark.parametrize("name,args", [("rgcn_resample_curves", CURVES), ("rgcn_resample_ranks", RANKS)])
def test_a_pointer_below_its_alignment_is_refused(name, args):
    """after every other check and before the first HIP call: the set passes everything else, so exactly
    RGCN_ERR_ALIGN comes back; the fully aligned set is never called - that would be a launch"""
    failed = S.misaligned_refusals(getattr(_lib.load(), name), name, args)
    assert not failed, "; ".join(failed)


def test_sizes_are_refused_before_any_launch():
    lib = _lib.load()
    A, RANGE = _lib.RGCN_ERR_ARG, _lib.RGCN_ERR_RANGE
    curves, ranks, weights = lib.rgcn_resample_curves, lib.rgcn_resample_ranks, lib.rgcn_resample_weights
    big = 2 ** 28 + 1
    # p3 = n, p4 = cut, p5 = num_units, p6 = replicates of the curves; p2 = m, p4 = nk, p5 = num_units, p6 = replicates
    assert curves(*_values(CURVES, p3=big, p4=0)) == RANGE and curves(*_values(CURVES, p6=65536)) == RANGE
    assert curves(*_values(CURVES, p5=2 ** 31)) == RANGE
    assert ranks(*_values(RANKS, p2=big)) == RANGE and ranks(*_values(RANKS, p6=65536)) == RANGE
    assert ranks(*_values(RANKS, p4=9)) == RANGE and ranks(*_values(RANKS, p5=2 ** 31)) == RANGE
    out = S.FAKE_BASE + S.FAKE_STEP
    assert weights(1, 65536, 0, out, None) == RANGE and weights(2 ** 31, 1, 0, out, None) == RANGE
    for bad in (dict(p3=-1), dict(p4=-1), dict(p4=2), dict(p5=0), dict(p6=-1), dict(p0=None), dict(p1=None), dict(p2=None),
                dict(p8=None), dict(p9=None), dict(p10=None), dict(p11=None), dict(p12=None), dict(p13=None)):
        assert curves(*_values(CURVES, **bad)) == A, bad
    for bad in (dict(p2=-1), dict(p4=-1), dict(p5=0), dict(p6=-1), dict(p0=None), dict(p1=None), dict(p3=None), dict(p8=None),
                dict(p9=None), dict(p10=None), dict(p11=None)):
        assert ranks(*_values(RANKS, **bad)) == A, bad
    assert weights(0, 1, 0, out, None) == A and weights(1, -1, 0, out, None) == A and weights(1, 1, 0, None, None) == A
    # a misplaced pointer is still reported when a size is also out of range: the sizes come first
    assert curves(*_values(CURVES, 1, 4, p3=big, p4=0)) == RANGE


# ---------------------------------------------------------------------------------- wrappers and command lines
def test_wrappers_refuse_cpu_tensors_and_wrong_arguments_by_name(monkeypatch):
    scores, labels = torch.rand(6), torch.ones(6)
    ranks = torch.ones(6, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="scores is on cpu.*no CPU fallback"):
        ops.classification_counts(scores, labels)
    with pytest.raises(RuntimeError, match="ranks is on cpu.*no CPU fallback"):
        ops.rank_sums(ranks, None, (1, 10), 4, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resample_weights(4, 2, 0, device="cpu")
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.classification_counts([0.5], labels)
    with pytest.raises(ValueError, match="replicates"):
        ops.resample_weights(4, 65536, 0)
    with pytest.raises(ValueError, match="num_units"):
        ops.resample_weights(0, 1, 0)

    def need(name, t, dtype):
        if t.dtype != dtype:
            raise TypeError(f"{name} must be {dtype}, got {t.dtype}")

    monkeypatch.setattr(ops, "_need_gpu", need)
    with pytest.raises(TypeError, match="ranks"):
        ops.rank_sums(ranks.int(), None, (1,), 0, 0)
    with pytest.raises(ValueError, match="ranks"):
        ops.rank_sums(ranks.view(2, 3), None, (1,), 0, 0)
    with pytest.raises(ValueError, match="k_values"):
        ops.rank_sums(ranks, None, range(1, 10), 0, 0)
    with pytest.raises(TypeError, match="unit"):
        ops.rank_sums(ranks, torch.zeros(6, dtype=torch.int64), (1,), 0, 0)
    with pytest.raises(ValueError, match="unit"):
        ops.rank_sums(ranks, torch.zeros(5, dtype=torch.int32), (1,), 0, 0)


def test_counts_helpers_mark_the_undefined():
    i = lambda *v: torch.tensor(v, dtype=torch.int64)
    c = ops.ClassificationCounts(wp=i(2, 0, 3), wn=i(2, 4, 0), auc2=i(6, 0, 0), ap=torch.tensor([0.75, 0.0, 0.0], dtype=torch.float64),
                                 tp=i(1, 0, 3), fp=i(1, 0, 0))
    assert c.degenerate().tolist() == [False, True, True]
    assert c.auc_roc()[0] == 0.75 and torch.isnan(c.auc_roc()[1:]).all() and torch.isnan(c.auc_pr()[1:]).all()
    assert c.precision()[0] == 0.5 and torch.isnan(c.precision()[1]) and c.precision()[2] == 1.0
    assert c.recall()[0] == 0.5 and torch.isnan(c.recall()[1]) and c.recall()[2] == 1.0
    assert c.f1()[0] == 0.5 and torch.isnan(c.f1()[1]) and c.accuracy().tolist() == [0.5, 1.0, 1.0]
    s = ops.RankSums(i(4, 0), i(10, 0), i(2, 0).view(2, 1), torch.tensor([2.0, 0.0], dtype=torch.float64), (10,))
    assert s.mrr()[0] == 0.5 and s.mean_rank()[0] == 2.5 and s.hits(10)[0] == 0.5
    assert torch.isnan(s.mrr()[1]) and torch.isnan(s.hits(10)[1])


def test_bootstrap_is_off_by_default_on_both_command_lines():
    args = compare.parse_args(["--methods", "random"])
    assert args.bootstrap == 0 and args.bootstrap_seed == 0 and not args.by_frequency
    args = compare.parse_args(["--methods", "random", "--bootstrap", "1000", "--bootstrap_seed", "7"])
    assert (args.bootstrap, args.bootstrap_seed) == (1000, 7)
    args = evaluate.parse_args(["--model_path", "m.pt"])
    assert args.bootstrap == 0 and args.bootstrap_seed == 0
    assert evaluate.parse_args(["--model_path", "m.pt", "--bootstrap", "200"]).bootstrap == 200
    for bad in (["--methods", "random", "--bootstrap", "-1"], ["--methods", "random", "--bootstrap", "65536"],
                ["--methods", "random", "--by_frequency"]):
        with pytest.raises(SystemExit):
            compare.parse_args(bad)
    with pytest.raises(SystemExit):
        evaluate.parse_args(["--model_path", "m.pt", "--bootstrap", "-3"])
    with pytest.raises(ValueError, match="by_frequency"):
        compare.compare_methods({}, {}, {"num_nodes": 4}, "cpu", methods=("random",), by_frequency=True)
    assert "bootstrap" in evaluate.ModelEvaluator.__dict__


def test_the_table_gains_standard_errors_only_when_asked():
    m = {"mrr": 0.5, "hits@1": 0.2, "hits@10": 0.8, "hits@50": 0.9}
    cls = {"auc_roc": 0.75, "auc_pr": 0.7}
    plain = {"protocol": {"filtered": True, "type_constrained": False, "sides": "both", "test_triples": 5},
             "methods": {"random": {"ranking": m, "classification": cls}}}
    assert "±" not in compare.table_markdown(plain) and "| random | 0.7500 | 0.7000 | 0.5000 |" in compare.table_markdown(plain)
    v = np.linspace(0.4, 0.6, 11)
    vectors = {"random": {k: v for k in ("auc_roc", "auc_pr", "mrr", "hits@10")}, "degree": {k: v + 0.1 for k in ("auc_roc", "auc_pr", "mrr", "hits@10")}}
    asked = {"protocol": dict(plain["protocol"], bootstrap={"replicates": 10, "seed": 0}),
             "methods": {n: {"ranking": m, "classification": cls, "bootstrap": bootstrap.block(vectors[n], 0, 10, 0)} for n in vectors},
             "significance": bootstrap.significance(vectors)}
    table = compare.table_markdown(asked)
    se = np.std(v[1:], ddof=1)
    assert f"| random | 0.7500 ± {se:.4f} | 0.7000 ± {se:.4f} | 0.5000 ± {se:.4f} | 0.2000 |" in table
    assert "| mrr | random vs degree | -0.1000 |" in table and "| 0.1818 |" in table          # 2 * 1 / 11
