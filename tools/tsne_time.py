"""Measurement: the t-SNE projection (``ops.tsne``) at PrimeKG's node-type sizes and the whole graph (M = 5,593 / 6,282 /
19,051 / 30,926), d = 128: the neighbour search, the affinities and the joint matrix, ONE gradient at ``slices`` 0 / 1 / 2 /
4 / 8 / 16, one update, a whole 1,000-iteration run - and scikit-learn's ``TSNE()`` (Barnes-Hut, angle 0.5) on this box's
CPUs beside them (the thread count the environment allows, at most 16).  The rows are Gaussian blobs (12 centres) unless
``--model_path`` names a checkpoint (then the encoder's output on ``synth.primekg_like``).  Device events around repeats
after a warm-up, no profiler; the run: wall clock, synchronised.  Needs the GPU; prints a plain-text table.

    python tools/tsne_time.py > profiles/tsne_time.txt
    python tools/tsne_time.py --no-host --sizes 5593      # the device half alone, one size
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from primekg_rgcn_linkprediction_amd import ops

D, PERPLEXITY = 128, 30.0
SIZES = (5593, 6282, 19051, 30926)


def timed(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / reps


def rows(args, m, dev):
    if args.model_path:
        from primekg_rgcn_linkprediction_amd import evaluate as E, synth
        model, _ = E.load_model(args.model_path, dev)
        ei, et, _, _ = synth.primekg_like(seed=42)
        with torch.no_grad():
            return model.eval().encoder(ei.to(dev), et.to(dev)).float()[:m].contiguous()
    rng = np.random.default_rng(m)
    centres = rng.normal(0.0, 3.0, size=(12, D))
    x = centres[rng.integers(0, 12, size=m)] + rng.normal(size=(m, D))
    return torch.from_numpy(x.astype(np.float32)).to(dev)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model_path", default=None)
    p.add_argument("--no-host", action="store_true", help="skip scikit-learn")
    p.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    p.add_argument("--max_iter", type=int, default=1000)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tsne_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    threads = min(16, int(os.environ.get("OMP_NUM_THREADS", "16")))
    print(f"t-SNE, d = {D}, perplexity {PERPLEXITY:g}, k = {int(3 * PERPLEXITY + 1)}; rows: "
          f"{'encoder output of ' + args.model_path if args.model_path else 'Gaussian blobs, 12 centres'}")
    print("device events, mean of 5 after 2 warm-up calls; whole run and host: one call, wall clock")
    for m in args.sizes:
        x = rows(args, m, dev)
        k = min(m - 1, int(3 * PERPLEXITY + 1))
        print(f"\nM = {m}")
        ids, sqdist = ops.knn(x, k)
        print(f"  knn (top-k pass + refine)            {timed(lambda: ops.knn(x, k)):10.3f} ms")
        cond_p, _ = ops.tsne_affinities(sqdist, PERPLEXITY)
        print(f"  affinities (perplexity search)       {timed(lambda: ops.tsne_affinities(sqdist, PERPLEXITY)):10.3f} ms")
        rowptr, col, val = ops.tsne_joint(ids, cond_p)
        print(f"  joint P (torch ops), nnz {col.numel():9d}  {timed(lambda: ops.tsne_joint(ids, cond_p)):10.3f} ms")
        y = torch.randn(m, 2, generator=torch.Generator().manual_seed(0)).to(dev) * 10
        for slices in (0, 1, 2, 4, 8, 16):
            ws = ops.tsne_workspace(m, slices, dev)
            grad, z, kl = ops.tsne_gradient(y, rowptr, col, val, 1.0, slices, False, ws=ws)
            ms = timed(lambda: ops.tsne_gradient(y, rowptr, col, val, 1.0, slices, False, grad, z, kl, ws))
            print(f"  one gradient, slices {slices:2d}              {ms:10.3f} ms   ({m * (m - 1) / (ms * 1e-3):.3e} pairs/s)")
        ms = timed(lambda: ops.tsne_gradient(y, rowptr, col, val, 1.0, 0, True, grad, z, kl))
        print(f"  one gradient with the error          {ms:10.3f} ms")
        update, gains = torch.zeros_like(y), torch.ones_like(y)
        ws = ops.tsne_workspace(m, 1, dev)
        norm2 = ops.tsne_update(grad, y.clone(), update, gains, 0.8, 200.0, ws=ws)
        yy = y.clone()
        print(f"  one update                           {timed(lambda: ops.tsne_update(grad, yy, update, gains, 0.8, 200.0, 0.01, norm2, ws)):10.3f} ms")
        ops.tsne(x, perplexity=PERPLEXITY, max_iter=20)
        stages = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ops.tsne(x, perplexity=PERPLEXITY, max_iter=args.max_iter, timings=stages)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        print(f"  ops.tsne, {res.n_iter} iterations             {total:10.3f} s    KL {res.kl_divergence:.4f}  "
              + "  ".join(f"{name} {s:.3f} s" for name, s in stages.items()))
        if not args.no_host:
            from sklearn.manifold import TSNE
            from threadpoolctl import threadpool_limits
            xh = x.cpu().numpy()
            with threadpool_limits(limits=threads):
                t0 = time.perf_counter()
                host = TSNE(n_components=2, random_state=42, perplexity=PERPLEXITY, max_iter=args.max_iter, n_jobs=threads).fit(xh)
                print(f"  TSNE() on the host, {threads} threads        {time.perf_counter() - t0:10.3f} s    KL {host.kl_divergence_:.4f} "
                      f"(Barnes-Hut, angle 0.5; {host.n_iter_ + 1} iterations)")


if __name__ == "__main__":
    main()
