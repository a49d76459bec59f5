"""GPU tier of ``attribution.edge_attribution`` and what is built on it (``consumers.attributed_edges``,
``consumers.attribution_edge_score``, ``ModelEvaluator.explain(by="gradient")``) against a float64 restatement of the
two-layer model on the CPU in which every column carries a mask leaf ``m`` (``w = m / segment_sum(m)``, the construction
``test_edge_grad_host.py`` holds to the kernel's reference) and torch autograd gives ``ds / dm``.

The tolerance of the device path cannot be derived - the split-precision transforms sit in it - so it is MEASURED against
something that does not involve the device: the same restatement run in float32 on the CPU.  Both errors are normalised
by ``max |total|`` of the float64 restatement, and the device must stay within ``GATE_FACTOR`` times the float32
restatement's error (the layers are documented at a few fp32 ulps against float64; the factor covers two layers and
different summation orders).  The float32 restatement's error is recomputed by every run (it involves no device), so
the gate is never a number taken from the device; ``MEASURED`` below records both errors as first seen on an MI355X."""
import functools

import pytest
import torch

import complex_reference
from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import DrugDiseaseModel, attribution, consumers, evaluate, ops, synth

pytestmark = pytest.mark.gpu

GATE_FACTOR = 8.0
# case -> (device error, float32 restatement's error), both / max |total|, as first measured on an MI355X
MEASURED = {
    "distmult": (2.353e-07, 2.674e-07),          # ratio 0.88
    "complex": (5.095e-07, 2.562e-07),           # ratio 1.99 (two triples; 4.116e-07 = 1.61 with one)
    "distmult-bases": (3.961e-07, 2.232e-07),    # ratio 1.77
}
N, E, R, D_IN, D_HID = 300, 6000, 3, 64, 128
ISLAND = 280                                            # nodes [ISLAND, N) form a component of their own
CASES = {"distmult": ("distmult", None), "complex": ("complex", None), "distmult-bases": ("distmult", 2)}
H, T, REL = 3, 17, 1


def _graph():
    ei, et, _, _ = synth.uniform_graph(N, E, R, seed=5)
    off = (ei >= ISLAND).any(0)
    ei[:, off] = ISLAND + ei[:, off] % (N - ISLAND)
    ei[:, :40] = ei[:, 40:80]                            # duplicate columns: several columns name one pair
    et[:20] = et[40:60]
    return ei.contiguous(), et.contiguous()


def _restate(params, ei, et, heads, rels, tails, coeff, decoder, dtype):
    """-> (layer1, layer2, score): ds / dm of the two layers' masks by autograd, everything in ``dtype`` on the CPU"""
    p = {k: v.to(dtype) for k, v in params.items()}
    src, dst = ei
    seg = dst * R + et
    masks = [torch.ones(ei.size(1), dtype=dtype, requires_grad=True) for _ in range(2)]

    def layer(x, m, w, root, bias):
        weight = m / torch.zeros(N * R, dtype=dtype).index_add(0, seg, m)[seg]
        agg = torch.zeros(N * R, x.size(1), dtype=dtype).index_add(0, seg, weight.unsqueeze(1) * x[src])
        return torch.einsum("nri,rio->no", agg.view(N, R, -1), w) + x @ root + bias

    h1 = torch.relu(layer(p["x"], masks[0], p["w1"], p["root1"], p["bias1"]))
    h2 = layer(h1, masks[1], p["w2"], p["root2"], p["bias2"])
    h, r, t = h2[heads], p["rel"][rels], h2[tails]
    score = complex_reference.score(h, r, t) if decoder == "complex" else (h * r * t).sum(-1)
    (score * coeff.to(dtype)).sum().backward()
    return masks[0].grad, masks[1].grad, score.detach()


def _effective(conv):
    w = conv.weight.detach().double().cpu()
    if conv.num_bases is None:
        return w
    return torch.einsum("rb,bio->rio", conv.comp.detach().double().cpu(), w)


@functools.lru_cache(maxsize=None)
def _case(name):
    dev = need_gpu()
    decoder, bases = CASES[name]
    torch.manual_seed(sorted(CASES).index(name))
    model = DrugDiseaseModel(N, R, D_IN, D_HID, dropout=0.5, num_bases=bases, decoder=decoder)
    with torch.no_grad():
        for conv in (model.encoder.conv1, model.encoder.conv2):
            conv.bias.uniform_(-0.1, 0.1)
    model = model.to(dev).eval()
    ei, et = _graph()
    enc = model.encoder
    params = {"x": enc.node_embeddings.weight, "w1": _effective(enc.conv1), "root1": enc.conv1.root, "bias1": enc.conv1.bias,
              "w2": _effective(enc.conv2), "root2": enc.conv2.root, "bias2": enc.conv2.bias,
              "rel": model.decoder.relation_embeddings.weight}
    params = {k: v.detach().double().cpu() for k, v in params.items()}
    heads, rels, tails = torch.tensor([H, 41]), torch.tensor([REL, 2]), torch.tensor([T, 9])
    coeff = torch.tensor([1.0, -0.5])
    out = {"model": model, "ei": ei, "et": et, "dev": dev, "queries": (heads, rels, tails, coeff)}
    for label, q in (("two", slice(0, 2)), ("one", slice(0, 1))):
        args = (heads[q], rels[q], tails[q], coeff[q])
        ref64 = _restate(params, ei, et, *args, decoder, torch.float64)
        ref32 = _restate(params, ei, et, *args, decoder, torch.float32)
        got = attribution.edge_attribution(model, ei.to(dev), et.to(dev), heads[q], rels[q], tails[q], coeff=coeff[q].to(dev))
        torch.cuda.synchronize()
        out[label] = (ref64, ref32, {k: v.cpu() for k, v in got.items()})
    return out


def _errors(case, label):
    (l1, l2, _), (a1, a2, _), got = case[label]
    total = l1 + l2
    scale = float(total.abs().max())
    err32 = float(((a1 + a2).double() - total).abs().max()) / scale
    dev = max(float((got["total"].double() - total).abs().max()), float((got["layer1"].double() - l1).abs().max()),
              float((got["layer2"].double() - l2).abs().max())) / scale
    return dev, err32, scale


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_attribution_is_the_gradient_in_the_masks(name):
    case = _case(name)
    for label in ("two", "one"):
        dev, err32, scale = _errors(case, label)
        print(f"{name} / {label}: device error {dev:.3e}, float32 restatement's error {err32:.3e}, ratio {dev / err32:.2f}, "
              f"max |total| {scale:.3e}")
        ref64, _, got = case[label]
        assert got["total"].shape == (E,) and got["total"].dtype == torch.float32
        assert torch.equal(got["total"], got["layer1"] + got["layer2"])
        assert float((got["score"].double() - ref64[2]).abs().max()) <= 1e-5 * max(1.0, float(ref64[2].abs().max()))
        assert 0 < err32 < 1e-5
        assert dev <= GATE_FACTOR * err32


@pytest.mark.parametrize("name", sorted(CASES))
def test_edges_that_cannot_matter_get_exactly_zero(name):
    case = _case(name)
    got = case["one"][2]
    src, dst = case["ei"]
    ends = (dst == H) | (dst == T)
    assert bool((got["layer2"][~ends] == 0.0).all()) and bool((got["layer2"][ends] != 0.0).any())
    near = torch.zeros(N, dtype=torch.bool)
    near[[H, T]] = True
    near[src[ends]] = True
    assert bool((got["layer1"][~near[dst]] == 0.0).all()) and bool((got["layer1"][near[dst] & ~ends] != 0.0).any())
    island = dst >= ISLAND
    assert int(island.sum()) > 20 and bool((src[island] >= ISLAND).all()) and bool((got["total"][island] == 0.0).all())


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_top_edges_are_the_references_wherever_it_separates_them(name):
    case = _case(name)
    (l1, l2, _), _, got = case["one"]
    _, err32, scale = _errors(case, "one")
    total = l1 + l2
    want = torch.sort(total.abs(), descending=True, stable=True)
    top = consumers.attributed_edges(got, case["ei"], case["et"], 10)
    assert len(top) == 10 and all(len(e) == 5 for e in top)
    gap = 2 * GATE_FACTOR * err32 * scale
    clear = 0
    for i, (column, s, r, t, value) in enumerate(top):
        assert (s, r, t) == (int(case["ei"][0, column]), int(case["et"][column]), int(case["ei"][1, column]))
        assert value == float(got["total"][column])
        separated = (i == 0 or float(want.values[i - 1] - want.values[i]) > gap) and float(want.values[i] - want.values[i + 1]) > gap
        if separated:
            clear += 1
            assert column == int(want.indices[i])
    assert clear >= 3
    tied = {"total": torch.tensor([1.0, -2.0, 2.0, 0.5, -2.0])}
    ei5, et5 = torch.tensor([[0, 1, 2, 3, 4], [1, 2, 3, 4, 0]]), torch.zeros(5, dtype=torch.int64)
    assert [e[0] for e in consumers.attributed_edges(tied, ei5, et5, 4)] == [1, 2, 4, 0]


def _evaluator(case):
    ei, et = case["ei"], case["et"]
    return evaluate.ModelEvaluator(case["model"], {"edge_index": ei[:, :16], "edge_type": et[:16]},
                                   {"edge_index": ei, "edge_type": et, "num_nodes": N}, case["dev"])


def test_explain_by_gradient_ranks_paths_by_the_attribution():
    case = _case("distmult")
    dev = case["dev"]
    ev = _evaluator(case)
    pairs, rels = [(H, T), (41, 9)], [REL, 2]
    paths, counts, edges = ev.explain(pairs, k=5, max_len=3, by="gradient", relations=rels, top_edges=7)
    assert len(paths) == len(counts) == len(edges) == 2
    ei, et = case["ei"].to(dev), case["et"].to(dev)
    pg = ops.PathGraph(ei, et, N)
    held = set(zip(pg.out_src.tolist(), pg.out_dst.tolist()))
    for (h, t), r, per_pair, count, top in zip(pairs, rels, paths, counts, edges):
        attr = attribution.edge_attribution(case["model"], ei, et, [h], [r], [t])
        hop_score = consumers.attribution_edge_score(attr, pg, ei)
        want = [0.0] * pg.nnz
        for entry, value in zip(pg.column_entries(ei).tolist(), attr["total"].abs().tolist()):
            want[entry] = max(want[entry], value)
        assert hop_score.tolist() == want
        nodes, length, score, cnt = ops.paths_topk(pg, hop_score, torch.tensor([h], device=dev), torch.tensor([t], device=dev), 5, 3)
        assert count == cnt[0].cpu().tolist() and len(per_pair) == int((length[0] > 0).sum()) > 0
        for j, path in enumerate(per_pair):
            assert path["nodes"] == nodes[0, j, :path["length"] + 1].cpu().tolist() and path["score"] == float(score[0, j])
            assert path["nodes"][0] == h and path["nodes"][-1] == t
            assert all(hop in held for hop in zip(path["nodes"][:-1], path["nodes"][1:]))
        assert top == consumers.attributed_edges(attr, ei, et, 7) and len(top) == 7


def test_explain_by_cosine_is_what_it_was():
    case = _case("distmult")
    ev = _evaluator(case)
    pairs = [(H, T), (41, 9)]
    got = ev.explain(pairs, k=4, max_len=3)
    assert got == ev.explain(pairs, 4, 3, by="cosine")
    pg = ops.PathGraph(case["ei"].to(case["dev"]), case["et"].to(case["dev"]), N)
    assert got == consumers.connecting_paths(ev.embeddings(), pg, pairs, 4, 3, return_counts=True)


def test_what_is_not_attributed_is_refused():
    case = _case("distmult")
    model, dev = case["model"], case["dev"]
    ei, et = case["ei"].to(dev), case["et"].to(dev)
    g = ops.bucket(ei, et, N, R)
    ed = ops.EdgeDropout(g)
    try:
        with pytest.raises(NotImplementedError):
            attribution.edge_attribution(model, ei, et, [H], [REL], [T], graph=ed.view)
    finally:
        ed.destroy()
    model.train()
    try:
        with pytest.raises(ValueError):
            attribution.edge_attribution(model, ei, et, [H], [REL], [T])
    finally:
        model.eval()
    with pytest.raises(IndexError):
        attribution.edge_attribution(model, ei, et, [N], [REL], [T])
    with pytest.raises(ValueError):
        attribution.edge_attribution(model, ei, et, [H, T], [REL], [T])
    half = DrugDiseaseModel(N, R, D_IN, D_HID, gather_dtype=torch.float16).to(dev).eval()
    with pytest.raises(NotImplementedError):
        attribution.edge_attribution(half, ei, et, [H], [REL], [T])
