"""Diagnostic: score-ranked connecting paths (``ops.paths_topk``) on the PrimeKG-shaped synthetic
graph (30,926 nodes, 849,456 columns) for 100 pairs - 20 drugs (the 10 with the most neighbours, so that hubs are in, and
10 random ones) x their 5 best-scored diseases under an untrained model of the reference's size - against the
reference's own method on the same host: the ``networkx.DiGraph`` loop over the columns and ``all_simple_paths(cutoff=L)`` with a per-pair time cap (``explain_predictions.py:255-292``).

    python tools/paths_time.py [--out FILE.json] [--cap SECONDS] [--no-host]

Device times are event times around the launches (mean of the repetitions after a warm-up); host times are wall clock.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from primekg_rgcn_linkprediction_amd import DrugDiseaseModel, _lib, ops, synth
from primekg_rgcn_linkprediction_amd.evaluate import ModelEvaluator

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--cap", type=float, default=0.25, help="seconds of all_simple_paths per pair before it is cut off")
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--k", type=int, default=5)
args = ap.parse_args()

dev = torch.device("cuda:0")
ei, et, n, r = synth.primekg_like(seed=42)
full = {"edge_index": ei, "edge_type": et, "num_nodes": n, "num_relations": r}
torch.manual_seed(0)
model = DrugDiseaseModel(n, r).to(dev).eval()
ev = ModelEvaluator(model, full, full, dev, node_class=synth.primekg_like_node_classes())
cls = synth.primekg_like_node_classes()
drugs = torch.nonzero(cls == cls[synth.N_DISEASE]).view(-1)
by_degree = torch.argsort(torch.bincount(ei[0], minlength=n)[drugs], descending=True, stable=True)
rest = by_degree[10:][torch.randperm(drugs.numel() - 10, generator=torch.Generator().manual_seed(1))[:10]]
drugs = drugs[torch.cat([by_degree[:10], rest])]
ids, _ = ev.top_candidates("tail", drugs, torch.zeros_like(drugs), 5, novel=False, candidate_class=int(cls[0]))
pairs = torch.stack([drugs.view(-1, 1).expand(-1, 5).reshape(-1), ids.cpu().reshape(-1)], 1)
assert pairs.shape == (100, 2) and int(pairs.min()) >= 0
emb = ev.embeddings().contiguous()
eid, etd = ei.to(dev), et.to(dev)


def timed(fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / reps


out = {"nodes": n, "columns": int(ei.size(1)), "pairs": 100, "k": args.k}
t0 = time.perf_counter()
graph = ops.PathGraph(eid, etd, n)
torch.cuda.synchronize()
out["path_graph_first_ms"] = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
graph = ops.PathGraph(eid, etd, n)
torch.cuda.synchronize()
out["path_graph_ms"] = (time.perf_counter() - t0) * 1e3
out["unique_pairs"] = graph.nnz
deg_out, deg_in = graph.out_ptr[1:] - graph.out_ptr[:-1], graph.in_ptr[1:] - graph.in_ptr[:-1]
out["max_out_degree"], out["max_in_degree"] = int(deg_out.max()), int(deg_in.max())
out["edge_cosine_ms"] = timed(lambda: ops.edge_cosine(emb, graph), reps=10, warm=2)
cosine = ops.edge_cosine(emb, graph)
src, dst = pairs[:, 0].contiguous().to(dev), pairs[:, 1].contiguous().to(dev)
out["source_out_degree_max"], out["target_in_degree_max"] = int(deg_out[src].max()), int(deg_in[dst].max())
lib = _lib.load()
out["slices_auto"] = lib.rgcn_paths_workspace_bytes(100, args.k, 0) // lib.rgcn_paths_workspace_bytes(100, args.k, 1)
print(json.dumps(out), flush=True)

for max_len in (3, 4):
    t0 = time.perf_counter()
    nodes, length, score, count = ops.paths_topk(graph, cosine, src, dst, args.k, max_len)
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    res = {"first_call_ms": first * 1e3}
    res["paths_topk_ms"] = timed(lambda: ops.paths_topk(graph, cosine, src, dst, args.k, max_len), reps=5 if first < 0.5 else 1, warm=0)
    total = count.sum(1).cpu()
    res["paths_total"], res["paths_max_per_pair"] = int(total.sum()), int(total.max())
    res["paths_per_length"] = count.sum(0).cpu().tolist()
    # every query alone with the batch's slice count: the worst one shows what one hub costs
    alone = []
    for q in range(100):
        alone.append(timed(lambda: ops.paths_topk(graph, cosine, src[q:q + 1], dst[q:q + 1], args.k, max_len,
                                                  slices=out["slices_auto"]), reps=1, warm=0))
    order = sorted(range(100), key=lambda q: alone[q])
    res["single_query_ms_median"], res["single_query_ms_max"] = alone[order[50]], alone[order[-1]]
    worst = order[-1]
    res["worst_query"] = {"pair": pairs[worst].tolist(), "paths": int(total[worst]), "source_out_degree": int(deg_out[src[worst]]),
                          "target_in_degree": int(deg_in[dst[worst]])}
    for s in (1, 4, 64, 256):
        res[f"paths_topk_ms_slices_{s}"] = timed(lambda: ops.paths_topk(graph, cosine, src, dst, args.k, max_len, slices=s),
                                                 reps=1, warm=0)
    out[f"max_len_{max_len}"] = res
    print(json.dumps({f"max_len_{max_len}": res}), flush=True)

if not args.no_host:
    import signal

    import networkx as nx

    class CapReached(Exception):
        pass

    def cap_reached(*_):
        raise CapReached

    signal.signal(signal.SIGALRM, cap_reached)         # the search can go long between two paths: cut it from outside
    t0 = time.perf_counter()
    g = nx.DiGraph()
    g.add_nodes_from(range(n))
    for u, v, rel in zip(ei[0].tolist(), ei[1].tolist(), et.tolist()):
        g.add_edge(u, v, relation=rel)
    out["host_digraph_s"] = time.perf_counter() - t0
    for max_len in (3, 4):
        capped = found = 0
        t0 = time.perf_counter()
        for s, t in pairs.tolist():
            signal.setitimer(signal.ITIMER_REAL, args.cap)
            try:
                for _ in nx.all_simple_paths(g, source=s, target=t, cutoff=max_len):
                    found += 1
            except CapReached:
                capped += 1
            finally:
                signal.setitimer(signal.ITIMER_REAL, 0)
        out[f"host_all_simple_paths_s_max_len_{max_len}"] = time.perf_counter() - t0
        out[f"host_pairs_capped_max_len_{max_len}"] = capped
        out[f"host_paths_found_max_len_{max_len}"] = found
        out["host_cap_s"] = args.cap
print(json.dumps(out, indent=1))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
