"""Diagnostic: the ComplEx head against the DistMult head of the same build at the training shape (DESIGN.md section 7,
the ComplEx row): ``*_bce_fwd`` + ``distmult_bce_reduce`` + ``*_bce_bwd`` over 4,096 samples (2,048 positives and their
corruptions from the device sampler) at d = 128 on the PrimeKG-shaped synthetic graph's node and relation counts, one
shared entity table.  Both heads read three rows and write three contribution rows per sample, and share the scatter and
the relation tree, so they should cost about the same.

    python tools/complex_time.py [--out FILE.txt]

Times are event times around ``--reps`` back-to-back calls on one stream after a warm-up; the figure is the median of
``--runs`` such windows, the spread their minimum and maximum.  The two heads alternate window by window.
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
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("complex_time.py measures on the GPU: none found")
dev = torch.device("cuda:0")
D, POSITIVES = 128, 2048
ei, et, n, r = synth.primekg_like(num_edges=synth.PRIMEKG_EDGES, seed=42)
ei, et = ei.to(dev), et.to(dev)
gen = torch.Generator().manual_seed(0)
emb, rel = (torch.randn(n, D, generator=gen) * 0.1).to(dev), (torch.randn(r, D, generator=gen) * 0.1).to(dev)
rng = torch.tensor([1, 0], dtype=torch.int64).to(dev)
h, t, rr, labels = ops.sample_batch(ei, et, None, None, POSITIVES, 1, n, rng)
batch = h.numel()
one = torch.ones(1, device=dev)
gh, gr = torch.empty_like(emb), torch.empty_like(rel)


def step(fwd, bwd):
    scores, loss = fwd(emb, h, emb, t, rel, rr, labels, batch)
    ops.distmult_bce_reduce(loss, scores, labels)
    bwd(one, scores, labels, emb, h, emb, t, rel, rr, batch, gh, gh, gr, zero_tables=True)


def window(fn):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(args.reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / args.reps * 1e3          # microseconds


heads = {"distmult": lambda: step(ops.distmult_bce_fwd, ops.distmult_bce_bwd),
         "complex": lambda: step(ops.complex_bce_fwd, ops.complex_bce_bwd)}
for fn in heads.values():
    for _ in range(20):
        fn()
torch.cuda.synchronize()
ops.check_indices(dev)
times = {name: [] for name in heads}
for _ in range(args.runs):
    for name, fn in heads.items():
        times[name].append(window(fn))
med = {name: statistics.median(v) for name, v in times.items()}
lines = [f"head forward + mean + backward, {batch} samples ({POSITIVES} positives + corruptions), d = {D}, "
         f"{n} nodes, {r} relations, one shared table, zero_tables",
         f"event time per call over {args.reps} back-to-back calls, median (min, max) of {args.runs} windows, the heads alternating"]
for name, v in times.items():
    lines.append(f"  {name:9s} {med[name]:8.1f} us  ({min(v):.1f}, {max(v):.1f})")
lines.append(f"  complex / distmult = {med['complex'] / med['distmult']:.3f}")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
