"""Host restatement of the pair-neighbourhood contract (``include/rgcn_neighborhood.h``), written from its words with
Python sets over the arrays of an ``ops.PathGraph`` on the CPU, plus the cases the CPU and GPU tiers share.

* ``nbr(u) = out(u) | in(u)``; a node is present when either row is non-empty (a self loop counts).
* ``B_0(x) = {x}`` for a present x, else empty; a ball grows by the neighbours of its FRONTIER (the nodes the last round
  added - every earlier node's neighbours are inside already).  An id outside ``[0, N)`` has empty balls.
* ``distance``: the first j with t in ``B_j(s)``; ``common`` / ``union_nodes``: sizes of the AND / OR of the two final
  balls; ``union_edges``: the unique ``(u, v)`` pairs with both ends in the union; ``class_count``: the union's nodes per
  class in ``[0, num_classes)``; ``common_nodes``: the smallest ids of the intersection, then -1.
"""
import numpy as np
import torch

MAX_RADIUS = 4


class Structure:
    """the rows of a CPU ``PathGraph`` as numpy slices, and its unique pairs"""

    def __init__(self, graph):
        self.n = graph.num_nodes
        self.out_ptr, self.out_dst = graph.out_ptr.numpy(), graph.out_dst.numpy()
        self.in_ptr, self.in_src = graph.in_ptr.numpy(), graph.in_src.numpy()
        src = np.repeat(np.arange(self.n), np.diff(self.out_ptr))
        self.pairs = list(zip(src.tolist(), self.out_dst.tolist()))

    def out(self, u):
        return self.out_dst[self.out_ptr[u]:self.out_ptr[u + 1]].tolist()

    def inn(self, u):
        return self.in_src[self.in_ptr[u]:self.in_ptr[u + 1]].tolist()

    def present(self, x):
        return 0 <= x < self.n and (self.out_ptr[x + 1] > self.out_ptr[x] or self.in_ptr[x + 1] > self.in_ptr[x])


def balls(st, x, radius):
    """[B_0(x), ..., B_radius(x)] as sets"""
    if not st.present(x):
        return [set() for _ in range(radius + 1)]
    ball, frontier = {x}, {x}
    grown = [set(ball)]
    for _ in range(radius):
        reached = set()
        for u in frontier:
            reached.update(st.out(u))
            reached.update(st.inn(u))
        frontier = reached - ball
        ball |= frontier
        grown.append(set(ball))
    return grown


def restate(graph, sources, targets, radius=2, node_class=None, num_classes=0, common_cap=0):
    """-> dict of numpy arrays with the names, shapes and dtypes of ``ops.PairNeighborhood`` (``class_count`` /
    ``common_nodes`` None when the contract does not produce them)"""
    st = graph if isinstance(graph, Structure) else Structure(graph)
    q = len(sources)
    classes = node_class is not None and num_classes > 0
    res = {"ball": np.zeros((q, 2, MAX_RADIUS + 1), dtype=np.int64), "distance": np.full(q, -1, dtype=np.int32),
           "common": np.zeros(q, dtype=np.int64), "union_nodes": np.zeros(q, dtype=np.int64),
           "union_edges": np.zeros(q, dtype=np.int64),
           "class_count": np.zeros((q, num_classes), dtype=np.int64) if classes else None,
           "common_nodes": np.full((q, common_cap), -1, dtype=np.int32) if common_cap > 0 else None}
    cls = None if not classes else np.asarray(node_class).tolist()
    for i, (s, t) in enumerate(zip(sources, targets)):
        s, t = int(s), int(t)
        bs, bt = balls(st, s, radius), balls(st, t, radius)
        for j in range(radius + 1):
            res["ball"][i, 0, j], res["ball"][i, 1, j] = len(bs[j]), len(bt[j])
            if res["distance"][i] < 0 and t in bs[j]:
                res["distance"][i] = j
        both, either = bs[radius] & bt[radius], bs[radius] | bt[radius]
        res["common"][i], res["union_nodes"][i] = len(both), len(either)
        res["union_edges"][i] = sum(1 for u, v in st.pairs if u in either and v in either)
        if classes:
            for u in either:
                if 0 <= cls[u] < num_classes:
                    res["class_count"][i, cls[u]] += 1
        if common_cap > 0:
            smallest = sorted(both)[:common_cap]
            res["common_nodes"][i, :len(smallest)] = smallest
    return res


FIELDS = ("ball", "distance", "common", "union_nodes", "union_edges", "class_count", "common_nodes")


def assert_same(got, want, what=""):
    """``got``: an ``ops.PairNeighborhood``; ``want``: ``restate``'s dict - shape, dtype and every value"""
    for name in FIELDS:
        g, w = getattr(got, name), want[name]
        if w is None:
            assert g is None, f"{what}{name} should not be produced"
            continue
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}{name}: {g.dtype} {g.shape}, want {w.dtype} {w.shape}"
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError(f"{what}{name} differs in {int((g != w).sum())} places, first at {at.tolist()}: "
                                 f"{g[tuple(at)]} for {w[tuple(at)]}")


# ---------------------------------------------------------------------------------- shared cases
def columns(pairs):
    ei = torch.tensor(pairs, dtype=torch.int64).t().contiguous().reshape(2, -1)
    return ei, torch.zeros(ei.size(1), dtype=torch.int64)


# The hand graph, 10 nodes.  7 and 9 have no edge at all, 8 has a self loop only, (0, 1) is given twice.
#   0 <-> 1 -> 2 -> 3 (self loop),  4 -> 2,  5 -> 6,  8 -> 8
HAND_N = 10
HAND_EDGES = [(0, 1), (1, 2), (2, 3), (3, 3), (4, 2), (1, 0), (0, 1), (5, 6), (8, 8)]
HAND_CLASS = [0, 0, 1, 1, 2, 2, -1, 0, 5, 1]        # three classes asked for: 6 (negative) and 8 (too large) count nowhere
HAND_RADIUS, HAND_NUM_CLASSES, HAND_CAP = 2, 3, 2
# (s, t): ball sizes of s, of t (radius 0, 1, 2), distance, common, union nodes, union edges, class counts, common ids
HAND_QUERIES = [
    # B(0) = {0}, {0,1}, {0,1,2};  B(3) = {3}, {2,3}, {1,2,3,4};  3 is three hops from 0
    ((0, 3), [1, 2, 3], [1, 2, 4], -1, 2, 5, 6, [2, 2, 1], [1, 2]),
    # B(2) = {2}, {1,2,3,4}, {0,..,4}
    ((0, 2), [1, 2, 3], [1, 4, 5], 2, 3, 5, 6, [2, 2, 1], [0, 1]),
    # s == t on a node whose only edge is its self loop: the loop is the one induced edge; class 5 is not counted
    ((8, 8), [1, 1, 1], [1, 1, 1], 0, 1, 1, 1, [0, 0, 0], [8, -1]),
    # an untouched source: not in the reference's graph
    ((9, 0), [0, 0, 0], [1, 2, 3], -1, 0, 3, 3, [2, 1, 0], [-1, -1]),
    ((5, 6), [1, 2, 2], [1, 2, 2], 1, 2, 2, 1, [0, 0, 1], [5, 6]),
    # a target past the last node, a negative source: nothing is read for them
    ((4, 12), [1, 2, 4], [0, 0, 0], -1, 0, 4, 4, [1, 2, 1], [-1, -1]),
    ((-1, 5), [0, 0, 0], [1, 2, 2], -1, 0, 2, 1, [0, 0, 1], [-1, -1]),
    # untouched on both sides, s == t: distance stays -1 (B_0 is empty)
    ((7, 7), [0, 0, 0], [0, 0, 0], -1, 0, 0, 0, [0, 0, 0], [-1, -1]),
]


def hand_case():
    """-> (edge_index, edge_type, sources, targets, node_class int32)"""
    ei, et = columns(HAND_EDGES)
    pairs = torch.tensor([q[0] for q in HAND_QUERIES], dtype=torch.int64)
    return ei, et, pairs[:, 0].contiguous(), pairs[:, 1].contiguous(), torch.tensor(HAND_CLASS, dtype=torch.int32)


def hand_answer():
    """the written-out answer as ``restate`` returns it"""
    q = len(HAND_QUERIES)
    ball = np.zeros((q, 2, MAX_RADIUS + 1), dtype=np.int64)
    for i, (_, bs, bt, *_rest) in enumerate(HAND_QUERIES):
        ball[i, 0, :3], ball[i, 1, :3] = bs, bt
    col = lambda k, dtype: np.array([row[k] for row in HAND_QUERIES], dtype=dtype)
    return {"ball": ball, "distance": col(3, np.int32), "common": col(4, np.int64), "union_nodes": col(5, np.int64),
            "union_edges": col(6, np.int64), "class_count": col(7, np.int64), "common_nodes": col(8, np.int32)}


def zipf_case(n, e=1500, seed=0, isolated=5, num_queries=40):
    """E columns whose endpoints are drawn with probability ~ 1 / (1 + rank) over a shuffled ranking of the first
    n - isolated nodes (a few hubs, many leaves, duplicate columns), six self loops; the last ``isolated`` ids have no
    edge.  Queries: random pairs, hubs, s == t, a repeated pair, isolated nodes, and ids outside [0, n).
    -> (edge_index, edge_type, sources, targets)"""
    gen = torch.Generator().manual_seed(seed)
    live = n - isolated
    rank = torch.randperm(live, generator=gen)
    prob = 1.0 / (1.0 + torch.arange(live, dtype=torch.float64))
    ends = rank[torch.multinomial(prob, 2 * e, replacement=True, generator=gen)].view(2, e)
    loops = rank[torch.randint(0, live, (6,), generator=gen)]
    ends[:, :6] = loops
    et = torch.randint(0, 3, (e,), generator=gen)
    pairs = torch.randint(0, n, (num_queries, 2), generator=gen)
    hub, second = int(rank[0]), int(rank[1])
    special = torch.tensor([[hub, second], [hub, hub], [int(loops[0]), int(loops[0])], [n - 1, hub], [hub, n - 1],
                            [n - 1, n - 2], [-1, hub], [hub, n], [n + 5, -7], [1 << 40, hub], [hub, second]], dtype=torch.int64)
    pairs[:special.size(0)] = special
    pairs[-1] = pairs[-2]                                                       # a repeated query
    return ends, et, pairs[:, 0].contiguous(), pairs[:, 1].contiguous()


def hub_case(m, seed=0):
    """Node 0 with an OUT-row of exactly m entries (0 -> 1..m) and node m + 1 with an IN-row of exactly m entries
    (1..m -> m + 1); a second pair of hubs the other way round (m + 2 with an in-row from the leaves m + 4 .. 2m + 3,
    m + 3 with an out-row to them) shares no node with the first; a few leaf-to-leaf columns; the last three ids
    untouched.  Queries: hub to hub (the first round walks one long out-row and one long in-row; the edge count walks the
    long out-row as a union member), leaf to leaf (the second round meets long and short rows in the same wave), across
    the two components, hub to itself.  -> (edge_index, edge_type, sources, targets, num_nodes)"""
    gen = torch.Generator().manual_seed(seed + m)
    a = torch.arange(1, m + 1)
    b = torch.arange(m + 4, 2 * m + 4)
    n = 2 * m + 4 + 3
    among = torch.stack([a[torch.randint(0, m, (20,), generator=gen)], a[torch.randint(0, m, (20,), generator=gen)]])
    ei = torch.cat([torch.stack([torch.zeros_like(a), a]), torch.stack([a, torch.full_like(a, m + 1)]),
                    torch.stack([b, torch.full_like(b, m + 2)]), torch.stack([torch.full_like(b, m + 3), b]), among], 1)
    et = torch.zeros(ei.size(1), dtype=torch.int64)
    pairs = torch.tensor([[0, m + 1], [1, m], [m + 2, m + 3], [m + 4, 2 * m + 3], [0, m + 2], [3, m + 7], [0, 0],
                          [m + 3, m + 3], [n - 1, 0]], dtype=torch.int64)
    return ei, et, pairs[:, 0].contiguous(), pairs[:, 1].contiguous(), n


COMMON_CAPS = (1, 64, 1024)
COMMON_SIZES = sorted({size for cap in COMMON_CAPS for size in (0, cap - 1, cap, cap + 65)})


def common_case(seed=3):
    """One (s, t) pair per size in COMMON_SIZES whose radius-1 intersection has exactly that many nodes: s and t each
    have an edge to every one of them and one private neighbour, and are not adjacent.  All ids come from one random
    permutation of 20,011 ids (626 bitset words), so an intersection's ids are scattered over all of them.
    -> (edge_index, edge_type, sources, targets, num_nodes)"""
    total = sum(COMMON_SIZES) + 4 * len(COMMON_SIZES)
    n = 20011
    assert total <= n
    ids = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).tolist()
    cols, pairs, at = [], [], 0
    for k, size in enumerate(COMMON_SIZES):
        s, t, ps, pt = ids[at:at + 4]
        shared = ids[at + 4:at + 4 + size]
        at += 4 + size
        cols += [(s, ps), (pt, t)]
        for j, c in enumerate(shared):                                         # both directions occur on both sides
            cols += [(s, c) if j % 2 else (c, s), (c, t) if j % 3 else (t, c)]
        pairs.append((s, t))
    ei, et = columns(cols)
    pairs = torch.tensor(pairs, dtype=torch.int64)
    return ei, et, pairs[:, 0].contiguous(), pairs[:, 1].contiguous(), n
