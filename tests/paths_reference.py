"""Host restatement of the path search's contract (``include/rgcn_paths.h``), written from its words, plus the cases the
CPU and GPU tiers share.

* The structure is what ``networkx.DiGraph.add_edge`` in a loop over the columns builds: unique ``(src, dst)`` pairs, the
  relation of the LAST column that names a pair; out-entries ordered by src, then dst.
* A path of length L is ``s = n0 -> ... -> nL = t`` along pairs of the structure with all L + 1 nodes distinct,
  ``1 <= L <= max_len``; ``s == t`` has none.
* ``score = (((c1 + c2) + c3) + c4)[first L terms] * float32(1 / (L * (1 + 0.2 * (L - 1))))``, every operation rounded
  to float32, ``c_i`` the edge score of hop i.
* ``count[L - 1]``: all simple paths of length L, NaN-scored ones included.  Listed are the k best without a NaN score
  by (score descending, L ascending, interior nodes ascending); empty slots are nodes -1, length 0, score -inf.
"""
import numpy as np
import torch

MAX_LEN = 4


def build_graph(edge_index, edge_type, num_nodes):
    """-> dict: ``pairs`` (the unique (u, v), sorted), ``pos`` {(u, v): index in pairs}, ``rel`` {(u, v): relation, last
    column wins}, ``succ`` {u: [v ascending]}"""
    ei, et = np.asarray(edge_index), np.asarray(edge_type)
    rel = {}
    for u, v, r in zip(ei[0].tolist(), ei[1].tolist(), et.tolist()):
        assert 0 <= u < num_nodes and 0 <= v < num_nodes
        rel[(u, v)] = r                                          # overwritten: the last one stays
    pairs = sorted(rel)
    succ = {}
    for u, v in pairs:
        succ.setdefault(u, []).append(v)
    return {"pairs": pairs, "pos": {p: i for i, p in enumerate(pairs)}, "rel": rel, "succ": succ, "num_nodes": num_nodes}


def enumerate_paths(graph, s, t, max_len=MAX_LEN):
    """every simple path from s to t of 1..max_len edges, as node tuples: a plain depth-first search with a visited set"""
    found = []
    if s == t:
        return found
    succ, path, seen = graph["succ"], [s], {s}

    def visit():
        for v in succ.get(path[-1], ()):
            if v == t:
                found.append(tuple(path) + (t,))
            elif v not in seen and len(path) < max_len:          # len(path) edges once v is added, one more to close
                path.append(v)
                seen.add(v)
                visit()
                seen.discard(path.pop())

    visit()
    return found


def path_weight(length):
    return np.float32(1.0 / (length * (1 + 0.2 * (length - 1))))


def path_score(graph, edge_score, path):
    """the contract's float32 score of one path"""
    hops = [np.float32(edge_score[graph["pos"][(u, v)]]) for u, v in zip(path[:-1], path[1:])]
    acc = hops[0]
    for c in hops[1:]:
        acc = np.float32(acc + c)
    return np.float32(acc * path_weight(len(hops)))


def restate_topk(graph, edge_score, sources, targets, k, max_len=MAX_LEN):
    """-> (nodes int32 [Q, k, 5], length int32 [Q, k], score float32 [Q, k], count int64 [Q, 4]) as numpy arrays"""
    edge_score = np.asarray(edge_score, dtype=np.float32)
    q = len(sources)
    nodes = np.full((q, k, MAX_LEN + 1), -1, dtype=np.int32)
    length = np.zeros((q, k), dtype=np.int32)
    score = np.full((q, k), -np.inf, dtype=np.float32)
    count = np.zeros((q, MAX_LEN), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, (s, t) in enumerate(zip(sources, targets)):
            ranked = []
            for path in enumerate_paths(graph, int(s), int(t), max_len):
                count[i, len(path) - 2] += 1
                sc = path_score(graph, edge_score, path)
                if not np.isnan(sc):
                    ranked.append((-float(sc), len(path) - 1, path[1:-1], path, sc))
            ranked.sort(key=lambda e: e[:3])
            for j, (_, hops, _, path, sc) in enumerate(ranked[:k]):
                nodes[i, j, :len(path)] = path
                length[i, j], score[i, j] = hops, sc
    return nodes, length, score, count


def same_bits(a, b):
    """float32 arrays equal bit for bit, except that -0.0 and +0.0 are one score"""
    a, b = np.asarray(a, dtype=np.float32) + np.float32(0), np.asarray(b, dtype=np.float32) + np.float32(0)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


# ---------------------------------------------------------------------------------- shared cases
RANDOM_N, RANDOM_E, RANDOM_Q, RANDOM_SEED, NUM_RELATIONS = 200, 2400, 37, 5, 3


def random_case():
    """N = 200, E = 2400 uniform random columns (duplicate pairs with different relations and self loops occur), 37
    random pairs -> (edge_index [2, E], edge_type [E], pairs [37, 2]) int64 tensors"""
    gen = torch.Generator().manual_seed(RANDOM_SEED)
    ei = torch.randint(0, RANDOM_N, (2, RANDOM_E), generator=gen)
    et = torch.randint(0, NUM_RELATIONS, (RANDOM_E,), generator=gen)
    pairs = torch.randint(0, RANDOM_N, (RANDOM_Q, 2), generator=gen)
    return ei, et, pairs


def random_embeddings(d, seed=7):
    """[200, d] float32; row 3 is zero (its edges score exactly 0.0)"""
    emb = torch.randn(RANDOM_N, d, generator=torch.Generator().manual_seed(seed))
    emb[3] = 0.0
    return emb


# The hand graph, 8 nodes (s = 0, t = 7).  Columns in this order; (0, 1) comes twice, relation 0 then 2.
HAND_EDGES = [
    (0, 1, 0), (0, 1, 2),      # the pair given twice: relation 2 stays
    (1, 0, 1),                 # the 2-cycle 0 <-> 1
    (1, 1, 0),                 # a self loop on an interior node
    (1, 7, 1),                 # 0 -> 1 -> 7
    (0, 7, 0),                 # the direct edge; with 7 -> 2 -> 7 below, 0 -> 7 -> 2 -> 7 is a walk through t, no path
    (7, 2, 1), (2, 7, 2),
    (0, 2, 1),                 # 0 -> 2 -> 7
    (1, 3, 0), (3, 7, 1),      # 0 -> 1 -> 3 -> 7
    (3, 2, 2),                 # 0 -> 1 -> 3 -> 2 -> 7
    (4, 5, 0),                 # 4 -> 5 is the only path from 4 to 5
    (5, 6, 1),                 # 6 has no way out: no path from 6 to anything
]
HAND_N = 8
# per-edge scores, chosen so that every sum of hops below is exact in float32 and the order is forced
HAND_SCORE = {(0, 1): 0.5, (1, 0): 0.25, (1, 1): 1.0, (1, 7): 0.5, (0, 7): 0.25, (7, 2): 1.0, (2, 7): 0.75, (0, 2): 0.25,
              (1, 3): 1.0, (3, 7): 0.5, (3, 2): 0.5, (4, 5): -0.5, (5, 6): 0.125}
# query -> ([(nodes, the exact sum of its hops' scores)], best first, and the number of paths per length); the score of a
# path is float32(sum) * path_weight(edges): w = 1, 0.41667, 0.238095, 0.15625
HAND_QUERIES = [
    ((0, 7), [((0, 1, 3, 7), 2.0),               # 0.47619
              ((0, 1, 3, 2, 7), 2.75),           # 0.42969
              ((0, 1, 7), 1.0),                  # 0.41667
              ((0, 2, 7), 1.0),                  # the same bits, the same length: interior node 1 before 2
              ((0, 7), 0.25)], [1, 2, 1, 1]),    # 0 -> 7 -> 2 -> 7 passes through t: not a path
    ((0, 0), [], [0, 0, 0, 0]),                  # s == t
    ((6, 0), [], [0, 0, 0, 0]),                  # no path: 6 has no way out
    ((4, 5), [((4, 5), -0.5)], [1, 0, 0, 0]),    # only the direct edge
    ((1, 7), [((1, 3, 7), 1.5),                  # 0.625
              ((1, 3, 2, 7), 2.25),              # 0.53571
              ((1, 7), 0.5),
              ((1, 0, 2, 7), 1.25),              # 0.29762
              ((1, 0, 7), 0.5)], [1, 2, 2, 0]),  # 0.20833; 1 -> 1 -> 7 and 1 -> 0 -> 1 -> 7 are no paths
]


def hand_case():
    """-> (edge_index, edge_type, pairs int64 tensors, edge_score float32 [nnz] in the structure's order)"""
    ei = torch.tensor([[u for u, _, _ in HAND_EDGES], [v for _, v, _ in HAND_EDGES]], dtype=torch.int64)
    et = torch.tensor([r for _, _, r in HAND_EDGES], dtype=torch.int64)
    pairs = torch.tensor([q for q, _, _ in HAND_QUERIES], dtype=torch.int64)
    return ei, et, pairs, torch.tensor([HAND_SCORE[p] for p in sorted(HAND_SCORE)], dtype=torch.float32)


def hand_answer(k):
    """the written-out answer as the arrays ``paths_topk`` returns"""
    q = len(HAND_QUERIES)
    nodes = np.full((q, k, MAX_LEN + 1), -1, dtype=np.int32)
    length = np.zeros((q, k), dtype=np.int32)
    score = np.full((q, k), -np.inf, dtype=np.float32)
    count = np.array([c for _, _, c in HAND_QUERIES], dtype=np.int64)
    for i, (_, paths, _) in enumerate(HAND_QUERIES):
        for j, (path, total) in enumerate(paths[:k]):
            nodes[i, j, :len(path)] = path
            length[i, j] = len(path) - 1
            score[i, j] = np.float32(np.float32(total) * path_weight(len(path) - 1))
    return nodes, length, score, count


def star_case(m):
    """A source 0 with m out-neighbours and a target 1 with m in-neighbours, m around the LDS staging limit, and few
    enough paths for the depth-first restatement: out(0) = A = {2 .. m + 1}, in(1) = B = {m / 2 + 2 .. m + m / 2 + 1}
    (the halves overlap: m / 2 paths of 2 edges), every a in A has an edge to three members of B (3-edge paths), a few
    to each other, and the first five members of A an edge back to 0.  Second query: (2, 1), a low-degree source against
    the same hub target.  Third query: (2, b) for a b in B with a handful of in-neighbours - its paths 2 -> 0 -> a -> b
    close the m entries of out(0) against that short in(b), the case where the lanes walk in(t) and search out(.).
    -> (edge_index, edge_type, pairs, num_nodes)"""
    gen = torch.Generator().manual_seed(m)
    a = torch.arange(2, m + 2)
    b = torch.arange(m // 2 + 2, m + m // 2 + 2)
    n = m + m // 2 + 2
    hops = torch.stack([a.repeat_interleave(3), b[torch.randint(0, m, (3 * m,), generator=gen)]])
    among = torch.stack([a[torch.randint(0, m, (m,), generator=gen)], a[torch.randint(0, m, (m,), generator=gen)]])
    back = torch.stack([a[:5], torch.zeros(5, dtype=torch.int64)])
    ei = torch.cat([torch.stack([torch.zeros_like(a), a]), torch.stack([b, torch.ones_like(b)]), hops, among, back], 1)
    et = torch.randint(0, NUM_RELATIONS, (ei.size(1),), generator=gen)
    return ei, et, torch.tensor([[0, 1], [2, 1], [2, int(hops[1, 30])]], dtype=torch.int64), n
