"""A planted graph for the learned edge masks and the float64 restatement of ``attribution.learn_edge_mask`` on the CPU
(no test lives here).  The score of the triple ``(HEAD, 0, TAIL)`` rests on FOUR planted columns: three in-edges of the
head inside a relation-0 segment of 80 edges (past the 64-edge border of the kernels) and one inside a relation-1 segment
of 6, all from SIGNAL nodes whose rows carry the only large entries of the table.  Every other in-edge of the head comes
from a node whose row is zero in the one coordinate the decoder reads, so it only dilutes the mean; the second layer's
bias is negative there, so the score is positive on the whole graph (0.19 x the tail's entry), larger when only the planted
columns are kept, and negative once they are deleted."""
import torch

N, R, D = 60, 2, 32                                           # (the cosine route takes rows of 32 k floats)
HEAD, TAIL, REL = 0, 1, 0
SIGNAL = [2, 3, 4, 5]
LONG = 80                                                     # in-edges of (HEAD, relation 0): 3 planted + 77 distractors


def graph(seed=7):
    """-> (edge_index [2, E], edge_type [E], planted columns (sorted list))"""
    gen = torch.Generator().manual_seed(seed)
    others = lambda k: torch.randint(10, N, (k,), generator=gen)              # noqa: E731  (neither signal nor the pair)
    parts = [(torch.tensor(SIGNAL[:3]), HEAD, 0), (others(LONG - 3), HEAD, 0),
             (torch.tensor(SIGNAL[3:]), HEAD, 1), (others(5), HEAD, 1),
             (others(12), TAIL, 0), (others(9), TAIL, 1)]
    src = torch.cat([p[0] for p in parts])
    dst = torch.cat([torch.full((p[0].numel(),), p[1]) for p in parts])
    rel = torch.cat([torch.full((p[0].numel(),), p[2]) for p in parts])
    m = 240                                                    # background: into the other nodes (the first layer's field)
    src = torch.cat([src, torch.randint(6, N, (m,), generator=gen)])
    dst = torch.cat([dst, torch.randint(10, N, (m,), generator=gen)])
    rel = torch.cat([rel, torch.randint(0, R, (m,), generator=gen)])
    planted_mask = torch.zeros(src.numel(), dtype=torch.bool)
    planted_mask[:3] = True
    planted_mask[LONG] = True
    order = torch.randperm(src.numel(), generator=gen)
    ei, et = torch.stack([src, dst])[:, order].contiguous(), rel[order].contiguous()
    planted = sorted(torch.nonzero(planted_mask[order]).view(-1).tolist())
    return ei, et, planted


def plant(model):
    """overwrite the parameters of a ``DrugDiseaseModel(N, R, D, D)`` (DistMult, no bases) with the planted ones"""
    gen = torch.Generator().manual_seed(1)
    enc = model.encoder
    with torch.no_grad():
        x = 0.05 * torch.randn(N, D, generator=gen)
        x[:, 0] = 0.0
        x[SIGNAL, 0] = 4.0
        x[TAIL, 0] = 2.0
        enc.node_embeddings.weight.copy_(x)
        eye = torch.eye(D)
        for conv, scale, bias0 in ((enc.conv1, 0.25, 0.0), (enc.conv2, 1.0, -0.15)):
            conv.weight.copy_(torch.stack([scale * eye, scale * eye]) + 0.01 * torch.randn(R, D, D, generator=gen))
            conv.root.copy_(eye)
            conv.bias.zero_()
            conv.bias[0] = bias0
        rel = torch.zeros(R, D)
        rel[:, 0] = 1.0
        model.decoder.relation_embeddings.weight.copy_(rel)
    return model


def parameters(model, dtype=torch.float64):
    enc = model.encoder
    p = {"x": enc.node_embeddings.weight, "w1": enc.conv1.weight, "root1": enc.conv1.root, "bias1": enc.conv1.bias,
         "w2": enc.conv2.weight, "root2": enc.conv2.root, "bias2": enc.conv2.bias,
         "rel": model.decoder.relation_embeddings.weight}
    return {k: v.detach().cpu().to(dtype) for k, v in p.items()}


def score_of(p, ei, et, m, head, rel, tail, n, r, decoder_score=None):
    """the two-layer score with every column's mask ``m`` entering both means as ``m / segment_sum(m)`` (a segment
    whose masks sum to 0 aggregates to zero), in ``m``'s dtype"""
    dtype = m.dtype
    src, dst = ei
    seg = dst * r + et
    total = torch.zeros(n * r, dtype=dtype).index_add(0, seg, m)[seg]
    w = torch.where(total > 0, m / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(m))

    def layer(x, weight, root, bias):
        agg = torch.zeros(n * r, x.size(1), dtype=dtype).index_add(0, seg, w.unsqueeze(1) * x[src])
        return torch.einsum("nri,rio->no", agg.view(n, r, -1), weight) + x @ root + bias

    h1 = torch.relu(layer(p["x"], p["w1"], p["root1"], p["bias1"]))
    h2 = layer(h1, p["w2"], p["root2"], p["bias2"])
    h, t, q = h2[head], h2[tail], p["rel"][rel]
    return decoder_score(h, q, t) if decoder_score is not None else (h * q * t).sum(-1)


def field_of(ei, head, tail, n):
    src, dst = ei
    ends = (dst == head) | (dst == tail)
    near = torch.zeros(n, dtype=torch.bool)
    near[src[ends]] = True
    near[[head, tail]] = True
    return near[dst]


def objective(p, ei, et, theta, cols, head, rel, tail, n, r, target, size_weight, entropy_weight, decoder_score=None):
    """-> (loss, score): ``learn_edge_mask``'s objective with ``theta`` a leaf, in ``theta``'s dtype"""
    m_field = torch.sigmoid(theta)
    m = torch.ones(ei.size(1), dtype=theta.dtype).index_put((cols,), m_field)
    score = score_of(p, ei, et, m, head, rel, tail, n, r, decoder_score)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(score, target.to(theta.dtype))
    mc = m_field.clamp(1e-12, 1.0 - 1e-12)
    entropy = -(mc * mc.log() + (1 - mc) * (1 - mc).log())
    return bce + size_weight * m_field.sum() + entropy_weight * entropy.mean(), score


def theta0(count, seed):
    return 1.0 + 0.1 * torch.randn(count, generator=torch.Generator().manual_seed(int(seed)))


def learn_restated(p, ei, et, head, rel, tail, n, r, steps=100, lr=0.1, size_weight=0.005, entropy_weight=1.0, seed=0,
                   dtype=torch.float64, decoder_score=None):
    """``learn_edge_mask`` in ``dtype`` on the CPU, the gradient by autograd -> (mask [E], field, first step's gradient)"""
    p = {k: v.to(dtype) for k, v in p.items()}
    e = ei.size(1)
    field = field_of(ei, head, tail, n)
    cols = torch.nonzero(field).view(-1)
    full = score_of(p, ei, et, torch.ones(e, dtype=dtype), head, rel, tail, n, r, decoder_score)
    target = (full >= 0).to(dtype)
    theta = theta0(cols.numel(), seed).to(dtype)
    avg, avg_sq, first = torch.zeros_like(theta), torch.zeros_like(theta), None
    for step in range(1, steps + 1):
        leaf = theta.clone().requires_grad_(True)
        loss, _ = objective(p, ei, et, leaf, cols, head, rel, tail, n, r, target, size_weight, entropy_weight, decoder_score)
        grad, = torch.autograd.grad(loss, leaf)
        first = grad if first is None else first
        avg = 0.9 * avg + 0.1 * grad
        avg_sq = 0.999 * avg_sq + 0.001 * grad * grad
        theta = theta - lr * (avg / (1 - 0.9 ** step)) / ((avg_sq / (1 - 0.999 ** step)).sqrt() + 1e-8)
    mask = torch.ones(e, dtype=dtype)
    mask[cols] = torch.sigmoid(theta)
    return mask, field, first
