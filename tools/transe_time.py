"""Diagnostic: the TransE baseline's training step and epoch (``ops.transe_step``, ``baselines.TransE``, DESIGN.md section
7 row 9) on the PrimeKG-shaped synthetic graph of ``bench.py`` (30,926 nodes, 849,456 columns: 830 batches of 1,024)
and at the train graph's column count, against the reference's own loop (``tests/transe_reference.py`` in the reference's
sample order, numpy float64) on the same host.

    python tools/transe_time.py [--out FILE.json] [--host-batches K] [--no-host] [--epochs N]

Device step times are event times around ``--reps`` back-to-back (sampler, step) pairs on one stream, after a warm-up;
the figure is the median of ``--runs`` such windows and the spread their minimum and maximum.  Epoch times are wall clock
around ``TransE.fit`` (which ends in a read-back) divided by its epochs, the first, which loads the code objects and may
capture the graph, left out by fitting twice with different epoch counts.  Host times are wall clock per batch; where a
host figure is multiplied out to an epoch or a run it is labelled an extrapolation.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import transe_reference as R
from primekg_rgcn_linkprediction_amd import baselines, ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--epochs", type=int, default=3, help="timed epochs per fit")
ap.add_argument("--host-batches", type=int, default=20)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--steps-only", action="store_true", help="only the step windows (for a kernel trace)")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("transe_time.py measures on the GPU: none found")
dev = torch.device("cuda:0")
D, BATCH, LR, MARGIN = 64, 1024, 0.01, 1.0
out = {"d": D, "batch": BATCH, "lr": LR, "margin": MARGIN,
       "protocol": f"event time over {args.reps} (sampler, step) pairs, median (min, max) of {args.runs} windows after a "
                   f"warm-up; epochs: wall clock of fit(1 + {args.epochs} epochs) minus fit(1 epoch), per epoch"}


def window(fn, reps):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / reps * 1e3          # microseconds


def fit_seconds(ei, et, n, r, epochs, hip_graph):
    model = baselines.TransE(D, epochs, LR, MARGIN, BATCH, seed=0, device=dev, hip_graph=hip_graph)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.fit(ei, et, n, r)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, model


for label, edges in (("primekg_like", synth.PRIMEKG_EDGES), ("train_graph_columns", synth.PRIMEKG_TRAIN_EDGES)):
    ei, et, n, r = synth.primekg_like(num_edges=edges, seed=42)
    ei, et = ei.to(dev), et.to(dev)
    res = {"nodes": n, "columns": edges, "relations": r, "batches_per_epoch": -(-edges // BATCH)}
    share = torch.bincount(ei.reshape(-1), minlength=n).max().item() / (2 * edges)
    res["busiest_node_share_of_endpoints"] = share
    res["busiest_node_slots_per_batch"] = share * 2 * BATCH * 1.5      # positives, and the corruption that keeps it
    if label == "primekg_like":
        gen = torch.Generator().manual_seed(0)
        emb, rel = baselines._unit_rows(n, D, gen).to(dev), baselines._unit_rows(r, D, gen).to(dev)
        order = torch.randperm(edges, device=dev)
        cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        rng = torch.tensor([1, 0], dtype=torch.int64).to(dev)
        loss_sum, active_sum = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)

        def pair():
            h, t, rr, _ = ops.sample_batch(ei, et, order, cursor, BATCH, 1, n, rng)
            ops.transe_step(emb, rel, h, t, rr, BATCH, LR, MARGIN, loss_sum, active_sum)

        h, t, rr, _ = ops.sample_batch(ei, et, order, cursor, BATCH, 1, n, rng)
        step_only = lambda: ops.transe_step(emb, rel, h, t, rr, BATCH, LR, MARGIN, loss_sum, active_sum)
        graph = torch.cuda.CUDAGraph()
        pair()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            pair()
        for name, fn in (("sampler_and_step_eager_us", pair), ("step_eager_us", step_only), ("sampler_and_step_replayed_us", graph.replay)):
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            times = sorted(window(fn, args.reps) for _ in range(args.runs))
            res[name] = {"median": statistics.median(times), "min": times[0], "max": times[-1]}
            print(json.dumps({name: res[name]}), flush=True)
        if args.steps_only:
            out[label] = res
            break
    for mode, hip_graph in (("eager", False), ("replayed", True)):
        one, _ = fit_seconds(ei, et, n, r, 1, hip_graph)
        more, model = fit_seconds(ei, et, n, r, 1 + args.epochs, hip_graph)
        res[f"epoch_{mode}_s"] = (more - one) / args.epochs
        res[f"first_epoch_{mode}_s"] = one
        res[f"losses_{mode}"] = model.epoch_losses
        res[f"active_{mode}"] = model.epoch_active
        print(json.dumps({f"{label}_epoch_{mode}_s": res[f"epoch_{mode}_s"], "losses": model.epoch_losses}), flush=True)
    res["eager_and_replayed_agree_bit_for_bit"] = res["losses_eager"] == res["losses_replayed"]
    out[label] = res

if not args.no_host and not args.steps_only:
    ei, et, n, r = synth.primekg_like(num_edges=synth.PRIMEKG_EDGES, seed=42)
    ei, et = ei.numpy(), et.numpy()
    R.fit(ei, et, n, r, D, 1, BATCH, LR, MARGIN, 0, "sample", max_batches=2)
    t0 = time.perf_counter()
    R.fit(ei, et, n, r, D, 1, BATCH, LR, MARGIN, 0, "sample", max_batches=args.host_batches)
    per_batch = (time.perf_counter() - t0) / args.host_batches
    t0 = time.perf_counter()
    init = R.init_tables(n, r, D, np.random.RandomState(0))
    setup = time.perf_counter() - t0
    out["host_sample_order"] = {
        "what": "tests/transe_reference.fit(order='sample'): the reference's per-sample loop in numpy float64, which like "
                "the reference renormalises the whole table after every batch",
        "batches_timed": args.host_batches, "s_per_batch": per_batch, "table_init_s": setup,
        "epoch_primekg_like_s_EXTRAPOLATED": per_batch * out["primekg_like"]["batches_per_epoch"],
        "fifty_epochs_train_graph_h_EXTRAPOLATED": per_batch * out["train_graph_columns"]["batches_per_epoch"] * 50 / 3600}
print(json.dumps(out, indent=1))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
