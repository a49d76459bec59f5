"""Diagnostic: what the relational attention layer costs (``attention.py``, ``ops.EdgeDropout.set_attention``,
``ops.edge_segment_sum``) on the PrimeKG-shaped synthetic graph of the true train-graph size
(C2: what tools/epoch_time.py trains on), against the mean layer.

    python tools/attention_time.py [--out FILE.txt]

Four things, on one GPU in one run: the attention draw (three launches) against the plain draw with the same window;
the per-segment edge sum in both directions; one layer's forward + backward at the encoder's two shapes, attention
against ``RGCNConv`` over the whole graph (what a trainer without the flag runs layer by layer); one trainer step
(``--attention --hide_batch_edges``, eager) against the eager and the captured step of the mean model with
``--hide_batch_edges``.  Times are event times around back-to-back calls on one stream after a warm-up, as many calls as
fill ``--window_ms`` (at least ``--reps``); the figure is the median of ``--runs`` such windows, the spread their
minimum and maximum; the things compared alternate window by window.
"""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from primekg_rgcn_linkprediction_amd import RGCNConv, ops, train as T
from primekg_rgcn_linkprediction_amd.attention import RelationalAttentionConv

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--window_ms", type=float, default=50.0)
ap.add_argument("--edges", type=int, default=1_708_556)      # 2 x 854,278 kg rows; ~1.68M train columns
ap.add_argument("--skip_step", action="store_true")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("attention_time.py measures on the GPU: none found")
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


def report(lines, res):
    for name, (med, lo, hi, reps) in res.items():
        lines.append(f"  {name:44s} {med:9.1f} us  ({lo:.1f}, {hi:.1f}; {reps} calls)")


tr, va, full, _ = T.synthetic_data(num_edges=args.edges, seed=42)
n, r = tr["num_nodes"], tr["num_relations"]
ei, et = tr["edge_index"].to(dev), tr["edge_type"].to(dev)
e = ei.size(1)
graph = ops.bucket(ei, et, n, r)
ed = ops.EdgeDropout(graph)
gen = torch.Generator().manual_seed(0)
order = torch.randperm(e, generator=gen).to(dev)
position = torch.empty(e, dtype=torch.int64, device=dev)
position[order] = torch.arange(e, device=dev)
rng, cursor, stats = torch.tensor([42, 1], device=dev), torch.tensor([4096], device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
batch = 1024
a = torch.randn(2, n, r, generator=gen).to(dev)

lines = [f"relational attention on the train graph of C2's size: {n:,} nodes, {r} relations, {e:,} train columns; longest "
         f"segment {int((graph.arrays(False)[0][1:] - graph.arrays(False)[0][:-1]).max()):,} (forward), "
         f"{int((graph.arrays(True)[0][1:] - graph.arrays(True)[0][:-1]).max()):,} (transposed) edges",
         f"event time per call over windows of >= {args.window_ms:.0f} ms of back-to-back calls, median (min, max) of "
         f"{args.runs} windows, the paths alternating"]
win = dict(cursor=cursor, batch=batch, position=position, stats=stats)
report(lines, compare({"plain draw, window of 1,024": lambda: ed.draw(0.0, rng, **win),
                       "attention draw, window of 1,024": lambda: ed.set_attention(a, 0.2, **win),
                       "  the same + HIDE_TWINS": lambda: ed.set_attention(a, 0.2, hide_twins=True, **win),
                       "attention draw, no window": lambda: ed.set_attention(a, 0.2)}))
values = torch.randn(e, generator=gen).to(dev)
report(lines, compare({"edge sum, (destination, relation)": lambda: ops.edge_segment_sum(graph, values),
                       "edge sum, (source, relation)": lambda: ops.edge_segment_sum(graph, values, transposed=True)}))

for d_in, d_out, relu in ((64, 128, True), (128, 128, False)):
    torch.manual_seed(1)
    mean, att = RGCNConv(d_in, d_out, r).to(dev), RelationalAttentionConv(d_in, d_out, r).to(dev)
    with torch.no_grad():
        att.att_dst.normal_(0, 0.1)
        att.att_src.normal_(0, 0.1)
    x = torch.randn(n, d_in, generator=gen).to(dev).requires_grad_(True)
    cot = torch.randn(n, d_out, generator=gen).to(dev)
    act = "relu" if relu else None

    def step(layer, **kw):
        x.grad = None
        layer.zero_grad(set_to_none=True)
        layer(x, ei, et, activation=act, **kw).backward(cot)

    lines.append(f"one layer, forward + backward, {d_in} -> {d_out}{' + ReLU' if relu else ''}")
    res = compare({"RGCNConv (mean)": lambda: step(mean), "RelationalAttentionConv": lambda: step(att, graph=graph)})
    report(lines, res)
    lines.append(f"  attention / mean: {res['RelationalAttentionConv'][0] / res['RGCNConv (mean)'][0]:.2f}")

if not args.skip_step:
    lines.append("one trainer step, batch 1,024 (64 -> 128 -> 128, Adam, --hide_batch_edges)")
    steps = {}
    for name, flags in (("mean model, captured step", []), ("mean model, eager (--no_hip_graph)", ["--no_hip_graph"]),
                        ("attention model, eager", ["--attention"])):
        targs = T.parse_args(["--hide_batch_edges", "--output_dir", tempfile.mkdtemp(), "--dropout", "0.0"] + flags)
        torch.manual_seed(0)
        trainer = T.Trainer(T.create_model(n, r, targs), tr, va, full, dev, targs)
        trainer.train_epoch(max_steps=8)                    # buckets, allocates the optimizer state, captures
        torch.cuda.synchronize()
        times = []
        for _ in range(args.runs):
            beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            beg.record()
            trainer.train_epoch(max_steps=40)
            end.record()
            torch.cuda.synchronize()
            times.append(beg.elapsed_time(end) / 40 * 1e3)
        steps[name] = (statistics.median(times), min(times), max(times), 40)
    report(lines, steps)
    lines.append("  (an epoch's fixed work - the permutation, the position scatter, the final read-back - is spread over its 40 steps)")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
