"""Measurement: k-means (R = 10 restarts, k = 10) and silhouette samples at PrimeKG's three node-type sizes
(``tests/golden/primekg_node_types.npz``: 19,051 genes, 6,282 drugs, 5,593 diseases), d = 128 - ``ops.kmeans`` and
``ops.silhouette_samples`` on the GPU, and scikit-learn's ``KMeans(n_init=10, random_state=42)`` and
``silhouette_score`` on this box's CPUs (the thread count the environment allows, at most 16).  The rows are random
normal unless ``--model_path`` names a checkpoint (then the encoder's output on ``synth.primekg_like``): random rows
have no cluster structure, so Lloyd runs long - the table therefore also gives the time per iteration.
Device events around repeats after a warm-up, no profiler.  Needs the GPU; prints one JSON document.

    python tools/cluster_time.py > profiles/cluster_time.json
    python tools/cluster_time.py --no-host            # the device half alone
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from primekg_rgcn_linkprediction_amd import ops

R, K, D = 10, 10, 128


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


def rows_by_type(args, dev):
    z = np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "primekg_node_types.npz"))
    cls, names = torch.from_numpy(z["node_class"].astype(np.int64)), [str(n) for n in z["class_names"]]
    if args.model_path:
        from primekg_rgcn_linkprediction_amd import evaluate as E, synth
        model, _ = E.load_model(args.model_path, dev)
        ei, et, _, _ = synth.primekg_like(seed=42)
        with torch.no_grad():
            emb = model.eval().encoder(ei.to(dev), et.to(dev)).float()
        source = f"encoder output of {args.model_path} on synth.primekg_like"
    else:
        emb = torch.randn(cls.numel(), D, generator=torch.Generator().manual_seed(0)).to(dev)
        source = "random normal rows, seed 0"
    return {name: emb[(cls == c).to(dev)].contiguous() for c, name in enumerate(names)}, source


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model_path", default=None)
    p.add_argument("--no-host", action="store_true", help="skip scikit-learn")
    p.add_argument("--max_iter", type=int, default=300)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/cluster_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    tables, source = rows_by_type(args, dev)
    threads = min(16, int(os.environ.get("OMP_NUM_THREADS", "16")))
    out = {"rows": source, "d": D, "restarts": R, "k": K, "max_iter": args.max_iter, "host_threads": threads,
           "timing": "device events, mean of 5 after 2 warm-up calls (whole k-means: 2 after 1); host: one call, wall clock",
           "types": {}}
    for name, x in sorted(tables.items(), key=lambda kv: -kv[1].size(0)):
        m = x.size(0)
        entry = {"M": m}
        init = ops.kmeans_plusplus(x, K, R, 42)
        entry["kmeans_plusplus_ms"] = timed(lambda: ops.kmeans_plusplus(x, K, R, 42))
        labels, changed = ops.kmeans_assign(x, init)
        entry["assign_ms"] = timed(lambda: ops.kmeans_assign(x, init, labels_prev=labels, labels=labels, num_changed=changed))
        centers = init.clone()
        entry["update_ms"] = timed(lambda: ops.kmeans_update(x, centers, labels, changed))
        entry["inertia_ms"] = timed(lambda: ops.kmeans_inertia(x, init, labels))
        fit = ops.kmeans(x, K, init=init, max_iter=args.max_iter)
        entry["kmeans_ms"] = timed(lambda: ops.kmeans(x, K, init=init, max_iter=args.max_iter), reps=2, warm=1)
        entry["kmeans_from_seed_ms"] = timed(lambda: ops.kmeans(x, K, n_init=R, seed=42, max_iter=args.max_iter), reps=2, warm=1)
        entry["kmeans_n_iter_of_winner"], entry["kmeans_inertia"] = fit.n_iter, fit.inertia
        for slices in (0, 1, 2, 4, 8, 16):
            key = "silhouette_samples_ms" if slices == 0 else f"silhouette_samples_ms_slices_{slices}"
            entry[key] = timed(lambda: ops.silhouette_samples(x, fit.labels, K, slices))
        entry["silhouette"] = ops.silhouette_score(x, fit.labels, K)
        entry["silhouette_pair_rate_per_s"] = m * m / (entry["silhouette_samples_ms"] * 1e-3)
        if not args.no_host:
            from sklearn.cluster import KMeans
            from sklearn.metrics import silhouette_score
            from threadpoolctl import threadpool_limits
            xh = x.cpu().numpy()
            with threadpool_limits(limits=threads):
                t0 = time.perf_counter()
                km = KMeans(n_clusters=K, n_init=R, random_state=42, max_iter=args.max_iter).fit(xh)
                entry["host_kmeans_s"] = time.perf_counter() - t0
                t0 = time.perf_counter()
                host_sil = float(silhouette_score(xh, fit.labels.cpu().numpy()))
                entry["host_silhouette_s"] = time.perf_counter() - t0
            entry["host_kmeans_n_iter"], entry["host_kmeans_inertia"] = int(km.n_iter_), float(km.inertia_)
            entry["host_silhouette_of_the_device_labels"] = host_sil
        out["types"][name] = entry
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
