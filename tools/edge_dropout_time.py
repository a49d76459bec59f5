"""Diagnostic: what edge dropout costs per training step (``ops.EdgeDropout``, csrc/edge_dropout.hip; DESIGN.md section 7
row 13) on the PrimeKG-shaped synthetic graph of the true train-graph size (C2: what tools/epoch_time.py trains on).

    python tools/edge_dropout_time.py [--out FILE.txt]

Four things, on one GPU in one run: rgcn_edge_dropout_create (it sorts the columns to pair the twins; wall time around
a synchronised call); the draw itself (three launches: p = 0.4 with the batch window, p = 0.4 alone, the window alone,
and the windowed draw with RGCN_EDGE_DROPOUT_HIDE_TWINS, with RGCN_EDGE_DROPOUT_PAIRED and with both); the forward gather over the view (weighted sums, 4 more bytes per edge) against the parent's
mean gather at the two widths of the encoder; the transposed gather over the view against the parent's (the same
kernel: the difference is the zeros among the weights).  Times are event times around back-to-back calls on one stream
after a warm-up, as many calls as fill ``--window_ms`` (at least ``--reps``); the figure is the median of ``--runs`` such
windows, the spread their minimum and maximum; the things compared alternate window by window.  The training step as a
whole is tools/epoch_time.py with and without ``--edge_dropout 0.4 --hide_batch_edges`` (and ``--hide_reverse_edges
--paired_edge_dropout`` on top).  ``--skip_gathers`` stops after the draws.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from primekg_rgcn_linkprediction_amd import ops, train as T

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--window_ms", type=float, default=50.0)
ap.add_argument("--edges", type=int, default=1_708_556)      # 2 x 854,278 kg rows; ~1.68M train columns
ap.add_argument("--skip_gathers", action="store_true")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("edge_dropout_time.py measures on the GPU: none found")
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


tr, _, _, _ = T.synthetic_data(num_edges=args.edges, seed=42)
n, r = tr["num_nodes"], tr["num_relations"]
ei, et = tr["edge_index"].to(dev), tr["edge_type"].to(dev)
e = ei.size(1)
graph = ops.BucketedGraph(ei, et, n, r)
create_ms = []
for _ in range(4):                                          # the first one warms the sorts up and is not reported
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ed = ops.EdgeDropout(graph)
    torch.cuda.synchronize()
    create_ms.append((time.perf_counter() - t0) * 1e3)
    if len(create_ms) < 4:
        ed.destroy()
view = ed.view
gen = torch.Generator().manual_seed(0)
order = torch.randperm(e, generator=gen).to(dev)
position = torch.empty(e, dtype=torch.int64, device=dev)
position[order] = torch.arange(e, device=dev)
rng, cursor, stats = torch.tensor([42, 1], device=dev), torch.tensor([4096], device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
batch = 1024

lines = [f"edge dropout on the train graph of C2's size: {n:,} nodes, {r} relations, {e:,} train columns; longest segment "
         f"{int((graph.arrays(False)[0][1:] - graph.arrays(False)[0][:-1]).max()):,} (forward), "
         f"{int((graph.arrays(True)[0][1:] - graph.arrays(True)[0][:-1]).max()):,} (transposed) edges",
         f"event time per call over windows of >= {args.window_ms:.0f} ms of back-to-back calls, median (min, max) of {args.runs} "
         f"windows, the paths alternating"]
lines.append(f"  rgcn_edge_dropout_create (wall, synchronised) {statistics.median(create_ms[1:]):8.2f} ms  "
             f"({min(create_ms[1:]):.2f}, {max(create_ms[1:]):.2f}; 3 calls after a first of {create_ms[0]:.2f} ms)")
windowed = lambda **kw: ed.draw(0.4, rng, cursor=cursor, batch=batch, position=position, stats=stats, **kw)   # noqa: E731
res = compare({"draw p = 0.4 + window of 1,024": windowed,
               "draw p = 0.4": lambda: ed.draw(0.4, rng, cursor=cursor, stats=stats),
               "draw window of 1,024 alone": lambda: ed.draw(0.0, rng, cursor=cursor, batch=batch, position=position, stats=stats),
               "  the same + HIDE_TWINS": lambda: windowed(hide_twins=True),
               "  the same + PAIRED": lambda: windowed(paired=True),
               "  the same + HIDE_TWINS + PAIRED": lambda: windowed(hide_twins=True, paired=True)})
# bytes the draw moves at least: perm (8) + segment id (4) + mark (4) per forward position; perm_t (8) + position (8, random)
# + segment id (4) + both weights written and the mark re-read (12) per edge in the second launch
need = e * (16 + 32)
for name, (med, lo, hi, reps) in res.items():
    lines.append(f"  {name:34s} {med:8.1f} us  ({lo:.1f}, {hi:.1f}; {reps} calls)  >= {need / med / 1e6:5.2f} TB/s of the {need / 2 ** 20:.0f} MiB it must move")
ed.draw(0.4, rng, cursor=cursor, batch=batch, position=position, stats=stats)
kept = int(ed.kept_counts().sum())
lines.append(f"  the view then keeps {kept:,} of {e:,} edges ({kept / e:.4f})")
stats.zero_()
windowed(hide_twins=True, paired=True)
lines.append(f"  with both options it keeps {int(ed.kept_counts().sum()):,} and hides {int(stats[1]):,} (the window's {batch:,} and their twins)")
for d in () if args.skip_gathers else (64, 128):
    x = torch.randn(n, d, generator=gen).to(dev)
    res = compare({"forward, parent (mean)": lambda: ops.aggregate(graph, x), "forward, view (p = 0.4)": lambda: ops.aggregate(view, x),
                   "transposed, parent": lambda: ops.aggregate(graph, x, transposed=True),
                   "transposed, view (p = 0.4)": lambda: ops.aggregate(view, x, transposed=True)})
    lines.append(f"gather, d = {d} (all levels, aggregate [{n:,}, {r * d}])")
    for name, (med, lo, hi, reps) in res.items():
        lines.append(f"  {name:34s} {med:8.1f} us  ({lo:.1f}, {hi:.1f}; {reps} calls)")
    lines.append(f"  view / parent: forward {res['forward, view (p = 0.4)'][0] / res['forward, parent (mean)'][0]:.3f}, "
                 f"transposed {res['transposed, view (p = 0.4)'][0] / res['transposed, parent'][0]:.3f}")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
