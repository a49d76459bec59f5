"""Diagnostic: the fused 1-vs-all softmax loss (``ops.softmax_lse`` + ``ops.softmax_grad``, csrc/softmax_loss.hip)
against the composition the package offered before it - ``ops.distmult_score_all_tails`` + ``torch.logsumexp`` + autograd
(two library GEMMs for the gradients) - on the same GPU in the same run (the softmax row).

    python tools/softmax_time.py [--out FILE.txt]

Shapes: B in {1024, 2048} queries against N in {30,926 (the drug / gene / disease subgraph), 129,375 (all of PrimeKG)}
candidates at d = 128, no mask (the masks cost one word load per row and 32 columns).  Times are event times around
back-to-back calls on one stream after a warm-up, as many calls as fill ``--window_ms`` (at least ``--reps``): a window
of a few calls would measure the clock and the scheduler.  The figure is the median of ``--runs`` such windows, the
spread their minimum and maximum; the two paths alternate window by window.  Peak memory is
``torch.cuda.max_memory_allocated`` over one call, above what the operands occupy.  A composition that does not fit is
recorded as such.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from primekg_rgcn_linkprediction_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--window_ms", type=float, default=50.0)
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("softmax_time.py measures on the GPU: none found")
dev = torch.device("cuda:0")
D = 128


def window(fn, reps):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / reps * 1e3               # microseconds


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


lines = [f"1-vs-all softmax loss, d = {D}, no mask: fused (softmax_lse; softmax_lse + softmax_grad with dq and dE) against",
         "the materialised composition (distmult_score_all_tails + torch.logsumexp; + autograd: two GEMMs)",
         f"event time per call over windows of >= {args.window_ms:.0f} ms of back-to-back calls, median (min, max) of "
         f"{args.runs} windows, the paths alternating"]
for n in (30926, 129375):
    for b in (1024, 2048):
        gen = torch.Generator().manual_seed(b + n)
        q = (torch.randn(b, D, generator=gen) * 0.1).to(dev)
        emb = (torch.randn(n, D, generator=gen) * 0.5).to(dev)
        target = torch.randint(0, n, (b,), generator=gen).to(dev)
        g = torch.full((b,), 1.0 / b, device=dev)
        ones, zero = torch.ones(1, D, device=dev), torch.zeros(b, dtype=torch.int64, device=dev)
        rows = torch.arange(b, device=dev)

        def fused_fwd():
            return ops.softmax_lse(q, emb, target, with_loss=True)

        def fused_both():
            lse = ops.softmax_lse(q, emb, target, with_loss=True)[0]
            return ops.softmax_grad(g, q, emb, target, lse)

        def mat_fwd():
            s = ops.distmult_score_all_tails(q, ones, zero, emb)[0]
            return torch.logsumexp(s, 1) - s[rows, target]

        def mat_both():
            s = ops.distmult_score_all_tails(q, ones, zero, emb)[0].requires_grad_(True)
            (torch.logsumexp(s, 1) - s[rows, target]).mean().backward()
            c = s.grad
            return c @ emb, c.t() @ q

        paths = {"fused forward": fused_fwd, "materialised forward": mat_fwd, "fused forward + backward": fused_both,
                 "materialised forward + backward": mat_both}
        fits = {}
        for name, fn in paths.items():
            try:
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                fits[name] = True
            except torch.OutOfMemoryError:
                fits[name] = False
                torch.cuda.empty_cache()
        times = {name: [] for name in paths if fits[name]}
        reps = {name: max(args.reps, int(args.window_ms * 1e3 / window(paths[name], args.reps)) + 1) for name in times}
        for _ in range(args.runs):
            for name in times:
                times[name].append(window(paths[name], reps[name]))
        flops = 2.0 * b * n * D
        lines.append(f"B = {b}, N = {n} (one score pass = {flops / 1e9:.1f} GFLOP, a [B, N] fp32 matrix = {b * n * 4 / 2 ** 20:.0f} MiB)")
        for name, fn in paths.items():
            if not fits[name]:
                lines.append(f"  {name:32s} does not fit")
                continue
            v = times[name]
            med = statistics.median(v)
            passes = 1 if name.endswith("forward") else 5
            lines.append(f"  {name:32s} {med:9.1f} us  ({min(v):.1f}, {max(v):.1f}; {reps[name]} calls)  {passes * flops / med / 1e6:6.1f} TFLOP/s of "
                         f"{passes} score pass{'es' if passes > 1 else ''}  peak {peak_above(fn):7.1f} MiB")
        if fits["materialised forward + backward"]:
            lines.append(f"  fused / materialised: forward {statistics.median(times['fused forward']) / statistics.median(times['materialised forward']):.2f}, "
                         f"forward + backward {statistics.median(times['fused forward + backward']) / statistics.median(times['materialised forward + backward']):.2f}")
        ops.check_indices(dev)
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
