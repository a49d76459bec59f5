"""Diagnostic: what the learned edge masks cost on C2's PrimeKG-shaped synthetic graph -

* the mask draw (``ops.EdgeDropout.set_mask``, csrc/edge_dropout.hip) beside the plain draw at ``p = 0``;
* the gradient through the view's normalisation (``ops.aggregate_weight_grad(through_normalisation=True)``,
  csrc/edge_grad.hip) beside the plain mode over the same view and the mean mode over the parent, at d = 64 and 128;
* one step and 100 steps of ``attribution.learn_edge_mask`` for a pair whose receptive field holds the longest segment.

    python tools/edge_mask_time.py [--out FILE.txt]

Kernel times are event times around back-to-back calls on one stream after a warm-up, as many calls as fill
``--window_ms`` (at least ``--reps``); the figure is the median of ``--runs`` such windows, the spread their minimum and
maximum; the paths compared alternate window by window.  ``learn_edge_mask`` is wall time around a synchronised call (it
builds its view, runs, and reads its losses back).  Nothing on the training path calls any of this: the figures are a
record (profiles/edge_mask.txt), not a gate.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from primekg_rgcn_linkprediction_amd import DrugDiseaseModel, attribution, ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--window_ms", type=float, default=50.0)
ap.add_argument("--edges", type=int, default=synth.PRIMEKG_EDGES)
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("edge_mask_time.py measures on the GPU: none found")
dev = torch.device("cuda:0")


def window(fn, reps):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / reps * 1e3               # microseconds


def compare(paths):
    """{name: fn} -> {name: (median, min, max, calls per window)}; the paths alternate window by window"""
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = {name: max(args.reps, int(args.window_ms * 1e3 / window(fn, args.reps)) + 1) for name, fn in paths.items()}
    times = {name: [] for name in paths}
    for _ in range(args.runs):
        for name, fn in paths.items():
            times[name].append(window(fn, reps[name]))
    return {name: (statistics.median(v), min(v), max(v), reps[name]) for name, v in times.items()}


ei, et, n, r = synth.primekg_like(num_edges=args.edges, seed=42)
ei, et = ei.to(dev), et.to(dev)
graph = ops.bucket(ei, et, n, r)
e = graph.num_edges
gen = torch.Generator().manual_seed(0)
rowptr = graph.arrays(False)[0].cpu().long()
lengths = rowptr[1:] - rowptr[:-1]
hub = int(lengths.argmax())
ed = ops.EdgeDropout(graph)
lines = [f"learned edge masks on C2's graph: {n:,} nodes, {r} relations, {e:,} columns; longest forward segment "
         f"{int(lengths.max()):,} edges (node {hub // r}, relation {hub % r}); forward weight bound of a view "
         f"{ed.view.weight_bound(False):.9f}",
         f"event time per call over windows of >= {args.window_ms:.0f} ms of back-to-back calls, median (min, max) of {args.runs} "
         f"windows, the paths alternating"]
rng = torch.zeros(2, dtype=torch.int64, device=dev)
mask = (torch.rand(e, generator=gen) * 0.98 + 0.01).to(dev)
res = compare({"plain draw, p = 0": lambda: ed.draw(0.0, rng), "mask draw": lambda: ed.set_mask(mask)})
lines.append("the draw into the view (three launches each)")
for name, (med, lo, hi, reps) in res.items():
    lines.append(f"  {name:44s} {med:8.1f} us  ({lo:.1f}, {hi:.1f}; {reps} calls)")
ed.set_mask(mask)
for d in (64, 128):
    x, gagg = torch.randn(n, d, generator=gen).to(dev), torch.randn(n, r * d, generator=gen).to(dev)
    res = compare({"weight gradient, plain (view)": lambda: ops.aggregate_weight_grad(ed.view, x, gagg),
                   "weight gradient through the mean (parent)": lambda: ops.aggregate_weight_grad(graph, x, gagg, through_mean=True),
                   "weight gradient through the normalisation": lambda: ops.aggregate_weight_grad(ed.view, x, gagg,
                                                                                                 through_normalisation=True)})
    lines.append(f"d = {d} (table [{n:,}, {d}], the aggregate's gradient [{n:,}, {r * d}], output float[{e:,}]; every call allocates "
                 f"its output)")
    for name, (med, lo, hi, reps) in res.items():
        lines.append(f"  {name:44s} {med:8.1f} us  ({lo:.1f}, {hi:.1f}; {reps} calls)")
ed.destroy()

torch.manual_seed(0)
model = DrugDiseaseModel(n, r, 64, 128, dropout=0.0).to(dev).eval()
head, tail = hub // r, int(ei[0, 0])
field = int(attribution.receptive_field(ei, head, tail, n).sum())
attribution.learn_edge_mask(model, ei, et, head, hub % r, tail, steps=2)       # warm-up: the passes are recorded here
torch.cuda.synchronize()
lines.append(f"attribution.learn_edge_mask for ({head}, {hub % r}, {tail}): {field:,} columns in the receptive field, 64 -> 128 "
             f"-> 128, wall time of a synchronised call, median (min, max) of {args.runs}")
for steps in (1, 100):
    walls = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        attribution.learn_edge_mask(model, ei, et, head, hub % r, tail, steps=steps)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"  {steps:3d} step(s) {statistics.median(walls):9.2f} ms  ({min(walls):.2f}, {max(walls):.2f})")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
