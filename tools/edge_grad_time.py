"""Diagnostic: what the gather's adjoint in its edge weights costs (``ops.aggregate_weight_grad``, csrc/edge_grad.hip;
DESIGN.md section 7 row 14) beside the forward gather at the same width on the same graph - C2's PrimeKG-shaped
synthetic graph at the two widths of the encoder, d = 64 and d = 128.

    python tools/edge_grad_time.py [--out FILE.txt]

The weight gradient reads the rows the gather reads and writes 4 bytes per edge instead of a row per segment, plus the
exchanges of the dot; the mean mode adds a second short launch over the dots.  Times are event times around
back-to-back calls on one stream after a warm-up, as many calls as fill ``--window_ms`` (at least ``--reps``); the
figure is the median of ``--runs`` such windows, the spread their minimum and maximum; the paths compared alternate
window by window.  No threshold is set here: the figures go to profiles/edge_grad.txt.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from primekg_rgcn_linkprediction_amd import ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--window_ms", type=float, default=50.0)
ap.add_argument("--edges", type=int, default=synth.PRIMEKG_EDGES)
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("edge_grad_time.py measures on the GPU: none found")
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
graph = ops.BucketedGraph(ei.to(dev), et.to(dev), n, r)
e = graph.num_edges
gen = torch.Generator().manual_seed(0)
longest = [int((graph.arrays(t)[0][1:] - graph.arrays(t)[0][:-1]).max()) for t in (False, True)]
lines = [f"the gather's adjoint in its edge weights on C2's graph: {n:,} nodes, {r} relations, {e:,} columns; longest segment "
         f"{longest[0]:,} (forward), {longest[1]:,} (transposed) edges",
         f"event time per call over windows of >= {args.window_ms:.0f} ms of back-to-back calls, median (min, max) of {args.runs} "
         f"windows, the paths alternating; every call allocates its output"]
for d in (64, 128):
    x, gagg = torch.randn(n, d, generator=gen).to(dev), torch.randn(n, r * d, generator=gen).to(dev)
    res = compare({"gather, forward (mean)": lambda: ops.aggregate(graph, x),
                   "weight gradient, forward": lambda: ops.aggregate_weight_grad(graph, x, gagg),
                   "weight gradient through the mean": lambda: ops.aggregate_weight_grad(graph, x, gagg, through_mean=True),
                   "gather, transposed": lambda: ops.aggregate(graph, x, transposed=True),
                   "weight gradient, transposed": lambda: ops.aggregate_weight_grad(graph, x, gagg, transposed=True)})
    lines.append(f"d = {d} (table [{n:,}, {d}], aggregate / its gradient [{n:,}, {r * d}], output float[{e:,}])")
    for name, (med, lo, hi, reps) in res.items():
        lines.append(f"  {name:34s} {med:8.1f} us  ({lo:.1f}, {hi:.1f}; {reps} calls)")
    fwd, bwd = res["gather, forward (mean)"][0], res["gather, transposed"][0]
    lines.append(f"  ratio to the gather of the same direction: plain forward {res['weight gradient, forward'][0] / fwd:.3f}, "
                 f"through the mean {res['weight gradient through the mean'][0] / fwd:.3f}, "
                 f"plain transposed {res['weight gradient, transposed'][0] / bwd:.3f}")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
