"""Diagnostic: the device bootstrap (``ops.classification_counts``, ``ops.rank_sums``) at the
size of PrimeKG's test split - a tenth of the graph's 849,456 columns: 84,945 triples, so 169,890 labelled scores (one
corruption each) and 169,890 ranks (both sides) - at 1,000 and 10,000 replicates, against scikit-learn's weighted
``roc_auc_score`` + ``average_precision_score`` on the same scores on the same host.

    python tools/resample_time.py [--out FILE.json] [--host-replicates K] [--no-host]
    rocprofv3 --kernel-trace --stats -d trace_dir -- python tools/resample_time.py --launches-only      # kernel times

Device times are event times around ``--reps`` back-to-back calls on one stream after a warm-up of the same shape; the
figure is the median of ``--runs`` such windows and the spread their minimum and maximum.  A call includes everything
the wrapper does (the sort, the gathers of labels and units, the tie flags, the one read-back of the cut).  The host
figure is wall clock per replicate over ``--host-replicates`` replicates; multiplied out to 1,000 replicates it is
labelled an extrapolation.  The reference has no bootstrap at all, so scikit-learn is what the device time is set against.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from primekg_rgcn_linkprediction_amd import bootstrap, ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--host-replicates", type=int, default=5)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--launches-only", action="store_true", help="a few calls of every shape and nothing else (for a kernel trace)")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("resample_time.py measures on the GPU: none found")
dev = torch.device("cuda:0")
TRIPLES = synth.PRIMEKG_EDGES // 10
K_VALUES = (1, 5, 10, 20, 50)
rng = np.random.RandomState(0)
labels_np = np.r_[np.ones(TRIPLES, np.int64), np.zeros(TRIPLES, np.int64)]
# scores of a fair model: positives above negatives on average, sigmoid outputs in float32 (ties are rare, as in a run)
scores_np = (1.0 / (1.0 + np.exp(-(rng.randn(2 * TRIPLES) + 1.5 * labels_np)))).astype(np.float32)
ranks_np = np.minimum(rng.geometric(0.01, 2 * TRIPLES), 30926).astype(np.int64)
scores, labels, ranks = (torch.from_numpy(a).to(dev) for a in (scores_np, labels_np, ranks_np))
score_unit = bootstrap.triple_units(TRIPLES, 2 * TRIPLES, dev)
rank_unit = bootstrap.query_units(TRIPLES, 2 * TRIPLES, dev)
out = {"test_triples": TRIPLES, "scores": 2 * TRIPLES, "ranks": 2 * TRIPLES, "k_values": list(K_VALUES),
       "protocol": f"event time over {args.reps} calls, median (min, max) of {args.runs} windows after a warm-up; a call is the "
                   f"whole wrapper (sort, gathers, tie flags, the read-back of the cut, the launch)"}


def window(fn, reps):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / reps          # milliseconds


for replicates in (1000, 10000):
    calls = {"classification_counts_ms": lambda: ops.classification_counts(scores, labels, score_unit, replicates, 1),
             "rank_sums_ms": lambda: ops.rank_sums(ranks, rank_unit, K_VALUES, replicates, 1)}
    res = {}
    for name, fn in calls.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        if args.launches_only:
            continue
        times = sorted(window(fn, args.reps) for _ in range(args.runs))
        res[name] = {"median": statistics.median(times), "min": times[0], "max": times[-1]}
        print(json.dumps({f"{name}@{replicates}": res[name]}), flush=True)
    out[f"replicates_{replicates}"] = res

if not args.no_host and not args.launches_only:
    from sklearn.metrics import average_precision_score, roc_auc_score
    counts = ops.classification_counts(scores, labels, score_unit, args.host_replicates, 1)
    weights = ops.resample_weights(TRIPLES, args.host_replicates, 1, device=dev).cpu().numpy()
    per, worst = [], 0.0
    for b in range(1, args.host_replicates + 1):
        w = weights[b][score_unit.cpu().numpy()].astype(np.float64)
        t0 = time.perf_counter()
        auc, apr = roc_auc_score(labels_np, scores_np, sample_weight=w), average_precision_score(labels_np, scores_np, sample_weight=w)
        per.append(time.perf_counter() - t0)
        worst = max(worst, abs(auc - float(counts.auc_roc()[b])), abs(apr - float(counts.auc_pr()[b])))
    out["host_scikit_learn"] = {
        "what": "roc_auc_score + average_precision_score(sample_weight = the device's own weights) per replicate, wall clock, "
                f"{os.cpu_count()} CPUs visible",
        "replicates_timed": args.host_replicates, "s_per_replicate_median": statistics.median(per),
        "s_per_replicate_min": min(per), "s_per_replicate_max": max(per),
        "s_per_1000_replicates_EXTRAPOLATED": statistics.median(per) * 1000,
        "largest_difference_from_the_device": worst}
print(json.dumps(out, indent=1))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
