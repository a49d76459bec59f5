"""Diagnostic: pair-neighbourhood statistics (``ops.pair_neighborhood``) on the PrimeKG-shaped
synthetic graph of ``bench.py`` (30,926 nodes, 849,456 columns) for 5,000 labelled pairs drawn the failure analysis'
way (``failures.sample_labelled_pairs``, seed 42), at radius 2 and radius 1, with three node classes and 16 common ids
per pair - against the reference's own method on the same host: the ``networkx.DiGraph`` loop over the columns and
``analyze_subgraph``'s set code (``analyze_failures.py:385-432``) over a stated sample of the same pairs.

    python tools/neighborhood_time.py [--out FILE.json] [--host-pairs K] [--no-host]

Device times are event times around ``--reps`` back-to-back calls, after a warm-up; the figure is the median of
``--runs`` such windows and the spread their minimum and maximum.  "Adjacency entries visited" is what the kernel's walk
reads by its own rules - both rows of every node of ``B_{r-1}`` of either end, and the out-row of every node of the
union - counted here by a separate dense breadth-first search in torch, which also has to reproduce the kernel's ball
and union sizes.  Host times are wall clock.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from primekg_rgcn_linkprediction_amd import failures, ops, synth

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--pairs", type=int, default=5000)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-pairs", type=int, default=20, help="pairs of the sample networkx analyses per radius")
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--edges", type=int, default=None, help="columns of the synthetic graph (default: PrimeKG's)")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("neighborhood_time.py measures on the GPU: none found")
dev = torch.device("cuda:0")
ei, et, n, r = synth.primekg_like(num_edges=args.edges or synth.PRIMEKG_EDGES, seed=42)
cls = synth.primekg_like_node_classes()                                 # 0 disease, 1 drug, 2 gene
pairs, labels = failures.sample_labelled_pairs(ei, cls, 1, 0, 2, args.pairs, seed=42)
pairs = torch.from_numpy(pairs)
graph = ops.PathGraph(ei.to(dev), et.to(dev), n)
src, dst, cls_dev = pairs[:, 0].contiguous().to(dev), pairs[:, 1].contiguous().to(dev), cls.to(dev)
deg_out, deg_in = graph.out_ptr[1:] - graph.out_ptr[:-1], graph.in_ptr[1:] - graph.in_ptr[:-1]
out = {"nodes": n, "columns": int(ei.size(1)), "unique_pairs": graph.nnz, "pairs": int(pairs.size(0)),
       "positives": int(labels.sum()), "max_out_degree": int(deg_out.max()), "max_in_degree": int(deg_in.max()),
       "hub_degree": ops.NEIGHBORHOOD_HUB_DEGREE, "lds_bytes_per_workgroup": 4 * ((n + 31) // 32) * 4,
       "protocol": f"event time over {args.reps} calls, median (min, max) of {args.runs} windows after 3 warm-up calls"}


def window(fn, reps):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / reps


def visited_entries(radius, chunk=500):
    """adjacency entries the walk reads per query (int64 [Q]) and the dense search's own ball / union sizes"""
    src_of = torch.repeat_interleave(torch.arange(n, device=dev), deg_out)
    dst_of = graph.out_dst.to(torch.int64)
    both = torch.cat([torch.stack([src_of, dst_of]), torch.stack([dst_of, src_of])], 1)
    adj = torch.sparse_coo_tensor(both, torch.ones(both.size(1), device=dev), (n, n)).coalesce().to_sparse_csr()
    total, present = (deg_out + deg_in).double(), ((deg_out + deg_in) > 0)
    visited, balls, unions = [], [], []
    for lo in range(0, pairs.size(0), chunk):
        reach, inner = [], []
        for ends in (src[lo:lo + chunk], dst[lo:lo + chunk]):
            x = torch.zeros(n, ends.numel(), device=dev)
            x[ends, torch.arange(ends.numel(), device=dev)] = present[ends].float()
            before = x
            for _ in range(radius):
                before, x = x, ((x + adj @ x) > 0).float()
            reach.append(x)
            inner.append(before if radius else torch.zeros_like(x))
        union = ((reach[0] + reach[1]) > 0).double()
        visited.append((total @ inner[0].double() + total @ inner[1].double() + deg_out.double() @ union).to(torch.int64))
        balls.append(torch.stack([reach[0].sum(0), reach[1].sum(0)], 1).to(torch.int64))
        unions.append(union.sum(0).to(torch.int64))
    return torch.cat(visited), torch.cat(balls), torch.cat(unions)


for radius in (2, 1):
    call = lambda s=src, t=dst: ops.pair_neighborhood(graph, s, t, radius, cls_dev, 3, 16)
    for _ in range(3):
        got = call()
    torch.cuda.synchronize()
    times = sorted(window(call, args.reps) for _ in range(args.runs))
    print(json.dumps({f"radius_{radius}_batch_ms": times}), flush=True)
    visited, balls, unions = visited_entries(radius)
    res = {"dense_search_agrees": torch.equal(balls, got.ball[:, :, radius]) and torch.equal(unions, got.union_nodes),
           "batch_ms_median": statistics.median(times), "batch_ms_min": times[0], "batch_ms_max": times[-1],
           "entries_visited": int(visited.sum()), "entries_per_s": float(visited.sum()) / (statistics.median(times) * 1e-3),
           "ball_mean": [float(got.ball[:, 0, radius].double().mean()), float(got.ball[:, 1, radius].double().mean())],
           "union_nodes_mean": float(got.union_nodes.double().mean()), "union_nodes_max": int(got.union_nodes.max()),
           "union_edges_mean": float(got.union_edges.double().mean()), "common_mean": float(got.common.double().mean())}
    # single queries: the 100 that visit most (the slowest is one of them) and 100 others for the typical cost
    heavy = torch.argsort(visited, descending=True)[:100].tolist()
    others = torch.randperm(pairs.size(0), generator=torch.Generator().manual_seed(1))[:100].tolist()
    alone = {}
    for q in heavy + others:
        one = lambda: call(src[q:q + 1], dst[q:q + 1])
        one()
        alone[q] = min(window(one, 5) for _ in range(3))
    worst = max(heavy, key=lambda q: alone[q])
    res["single_query_ms_typical"] = statistics.median(alone[q] for q in others)
    res["single_query_ms_slowest"] = alone[worst]
    res["slowest_query"] = {"pair": pairs[worst].tolist(), "entries_visited": int(visited[worst]),
                            "share_of_entries": float(visited[worst]) / float(visited.sum()),
                            "alone_over_batch": alone[worst] / res["batch_ms_median"],
                            "union_nodes": int(got.union_nodes[worst]), "degrees": [int((deg_out + deg_in)[pairs[worst, 0]]),
                                                                                    int((deg_out + deg_in)[pairs[worst, 1]])]}
    out[f"radius_{radius}"] = res
    print(json.dumps({f"radius_{radius}": res}), flush=True)

if not args.no_host:
    import networkx as nx

    t0 = time.perf_counter()
    g = nx.DiGraph()
    for u, v, rel in zip(ei[0].tolist(), ei[1].tolist(), et.tolist()):
        g.add_edge(u, v, relation=rel)
    out["host_digraph_s"] = time.perf_counter() - t0
    types = dict(enumerate(cls.tolist()))
    sample = torch.randperm(pairs.size(0), generator=torch.Generator().manual_seed(2))[:args.host_pairs].tolist()
    for radius in (2, 1):
        t0 = time.perf_counter()
        for q in sample:
            found = []
            for x in pairs[q].tolist():
                ball = set()
                if x in g:
                    ball.add(x)
                    for _ in range(radius):
                        new = set()
                        for node in list(ball):
                            new.update(g.successors(node))
                            new.update(g.predecessors(node))
                        ball.update(new)
                found.append(ball)
            union = found[0] | found[1]
            edges = g.subgraph(union).number_of_edges()
            counts = {}
            for node in union:
                counts[types.get(node)] = counts.get(types.get(node), 0) + 1
        seconds = time.perf_counter() - t0
        out[f"host_radius_{radius}"] = {"pairs": len(sample), "seconds": seconds, "ms_per_pair": seconds / len(sample) * 1e3,
                                        "device_ms_per_pair": out[f"radius_{radius}"]["batch_ms_median"] / pairs.size(0)}
print(json.dumps(out, indent=1))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
