"""Diagnostic: the ranking evaluation on the real PrimeKG test columns (15,372) over a
C2-sized graph: fused tail ranks (encode once + distmult_rank_tails) vs the reference's protocol
(evaluate.py:251-276: encoder per 1,024-edge batch, score_all_tails, per-edge argsort + nonzero().item())
timed on the first batches and scaled."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from primekg_rgcn_linkprediction_amd import DrugDiseaseModel, synth
from primekg_rgcn_linkprediction_amd.evaluate import ModelEvaluator

dev = torch.device("cuda:0")
z = np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "primekg_test_edges.npz"))
test = {"edge_index": torch.from_numpy(z["edge_index"]).long(), "edge_type": torch.from_numpy(z["edge_type"]).long(),
        "num_nodes": 30926, "num_relations": 3}
ei, et, n, r = synth.primekg_like(seed=42)
full = {"edge_index": ei, "edge_type": et, "num_nodes": n, "num_relations": r}
torch.manual_seed(0)
model = DrugDiseaseModel(n, r).to(dev).eval()
ev = ModelEvaluator(model, test, full, dev)
ev.tail_ranks(); torch.cuda.synchronize()                      # warm (bucketing)
ev._emb = None if hasattr(ev, "_emb") else None
t0 = time.perf_counter()
ev2 = ModelEvaluator(model, test, full, dev)
ranks = ev2.tail_ranks(); torch.cuda.synchronize()
t_fused = time.perf_counter() - t0
m = ev2.compute_ranking_metrics()
print(f"fused: {test['edge_index'].size(1)} test edges ranked in {t_fused * 1e3:.1f} ms (encoder once + one MFMA pass); "
      f"MRR {m['mrr']:.4f}")
# the two device passes by themselves (events): the no-grad encoder and the fused ranking launch
with torch.no_grad():
    emb = ev2.embeddings()
    head, tail, rel = ev2.test_edge_index[0], ev2.test_edge_index[1], ev2.test_edge_type
    hemb = emb[head]
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, fn in (("no-grad encoder", lambda: model.encoder(ev2.full_edge_index, ev2.full_edge_type)),
                     ("rank_tails (products, true scores, MFMA pass with the counting epilogue)",
                      lambda: model.decoder.rank_tails(hemb, rel, emb, tail)),
                     ("score_all_tails, first 1,024 edges ([1024, 30926] matrix)",
                      lambda: model.decoder.score_all_tails(hemb[:1024], rel[:1024], emb))):
        for _ in range(3):
            fn()
        beg.record()
        for _ in range(10):
            fn()
        end.record()
        torch.cuda.synchronize()
        print(f"    {name}: {beg.elapsed_time(end) / 10:.3f} ms")
# the reference's loop, first 2 batches of 1,024
eid, etd = ei.to(dev), et.to(dev)
heads, tails, rels = (t.to(dev) for t in (test["edge_index"][0], test["edge_index"][1], test["edge_type"]))
t0 = time.perf_counter(); done = 0; diffs = []
with torch.no_grad():
    for lo in range(0, 2048, 1024):
        emb = model.encoder(eid, etd)
        scores = model.decoder.score_all_tails(emb[heads[lo:lo + 1024]], rels[lo:lo + 1024], emb)
        for i in range(scores.size(0)):
            order = torch.argsort(scores[i], descending=True)
            rank = (order == tails[lo + i]).nonzero(as_tuple=True)[0].item() + 1
            diffs.append(abs(rank - int(ranks[lo + i])))
            done += 1
torch.cuda.synchronize()
t_ref = (time.perf_counter() - t0) / done * test["edge_index"].size(1)
print(f"reference protocol on the same kernels otherwise: {t_ref:.2f} s for all test edges (scaled from {done}); "
      f"ranks equal on {sum(d == 0 for d in diffs)} of those {done}, max |delta| {max(diffs)} "
      f"(two fp32 dot products of different summation order can swap neighbours whose scores agree to ~1e-7)")

# ---- filtered + type-constrained ranking at the same shape (B = 15,372, N = 30,926, d = 128): the masked pass, the
# mask builds, and what the same protocol costs without them - score_all_tails in slices of 1,024 queries + torch
# masking and counting with the same masks expanded to bool on the device beforehand
from primekg_rgcn_linkprediction_amd import ops


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / reps


with torch.no_grad():
    emb = ev2.embeddings().contiguous()
    head, tail, rel = ev2.test_edge_index[0], ev2.test_edge_index[1], ev2.test_edge_type
    cls = synth.primekg_like_node_classes().to(dev)
    known = ops.KnownTriples(torch.cat([ev2.full_edge_index, ev2.test_edge_index], 1),
                             torch.cat([ev2.full_edge_type, ev2.test_edge_type]), n, r)
    dec = model.decoder
    hr = (emb[head] * dec.relation_embeddings(rel)).contiguous()
    true = (hr * emb[tail]).sum(1)
    qcls = cls[tail].contiguous()
    allow = ops.class_allow_bits(cls, 3)
    excl = known.exclude_bits("tail", head, rel)
    t_raw_call = timed(lambda: dec.rank_tails(emb[head], rel, emb, tail))
    t_raw = timed(lambda: ops.distmult_rank_tails(hr, emb, true, tail))
    t_nomask = timed(lambda: ops.distmult_rank_masked(hr, emb, true, tail))
    t_masked = timed(lambda: ops.distmult_rank_masked(hr, emb, true, tail, allow, qcls, excl))
    t_excl = timed(lambda: known.exclude_bits("tail", head, rel, out=excl))
    t_allow = timed(lambda: ops.class_allow_bits(cls, 3))
    t_call = timed(lambda: dec.rank_tails(emb[head], rel, emb, tail, known=known, head_indices=head, node_class=cls))
    fused = ops.distmult_rank_masked(hr, emb, true, tail, allow, qcls, excl)

    shifts = torch.arange(32, device=dev, dtype=torch.int32)
    allow_b = ((allow.unsqueeze(2) >> shifts) & 1).bool().reshape(3, -1)[:, :n]

    def torch_route():
        out = []
        for lo in range(0, head.numel(), 1024):
            sl = slice(lo, lo + 1024)
            scores = dec.score_all_tails(emb[head[sl]], rel[sl], emb)
            keep = allow_b[qcls[sl].long()] & ~((excl[sl].unsqueeze(2) >> shifts) & 1).bool().reshape(scores.size(0), -1)[:, :n]
            beat = (scores > true[sl].unsqueeze(1)) & keep
            beat[torch.arange(scores.size(0), device=dev), tail[sl]] = False
            out.append(beat.sum(1) + 1)
        return torch.cat(out)

    t_torch = timed(torch_route, reps=3, warm=1)
    same = int((torch_route() == fused).sum())
print("filtered + type-constrained tail ranking, B = %d, N = %d, d = 128 (events, mean of 10):" % (head.numel(), n))
print(f"    (i)   rank_tails raw, whole call: {t_raw_call:.3f} ms; its ranking launch alone (distmult_rank_tails): {t_raw:.3f} ms")
print(f"    (ii)  masked pass alone, both masks (distmult_rank_masked): {t_masked:.3f} ms = {t_masked / t_raw:.2f} x the raw launch"
      f"; the same launch with no mask: {t_nomask:.3f} ms")
print(f"    (iii) mask builds: exclude [15372, 967] words {t_excl:.3f} ms (incl. the segment lookup), allow [3, 967] {t_allow:.3f} ms")
print(f"    (iv)  score_all_tails in slices of 1,024 + torch masking and counting with the same masks: {t_torch:.3f} ms")
print(f"    (ii)+(iii) = {t_masked + t_excl + t_allow:.3f} ms against (iv) {t_torch:.3f} ms: {t_torch / (t_masked + t_excl + t_allow):.1f} x; "
      f"rank_tails(known=, node_class=) whole call {t_call:.3f} ms; ranks equal on {same} of {head.numel()} "
      f"(the slices' true score is the same row-wise dot)")
