"""Small typed graphs for the sparse-aggregate tests (``test_sparse_aggregate.py``, ``test_sparse_aggregate_host.py``),
built the way ``hub_graphs.py`` builds its own: segment by segment from stated properties, then shuffled.  A plain
module, not a conftest.

Every graph has, in BOTH directions (destination side = the forward structure, source side = the transposed one):

  - relation ``EMPTY_REL`` without any edge;
  - relation 0 absent from one whole 64-row tile (``empty_tile(n)``: rows 64..127 where the graph has them, else rows
    0..63), so that a consumer skips that (tile, relation) block AND redirects single rows elsewhere;
  - node ``ISOLATED`` without an edge in any relation;
  - one segment of ``HUB_EDGES`` > 256 edges (a hub tail the gather may leave to its consumer) at node ``HUB`` in
    relation 1, in a 64-row tile about half of whose other segments are empty;
  - a ragged last tile: n is 150 or 70, a multiple of neither 32 nor 64.
About half of the remaining (node, relation) segments are empty, as on the knowledge graph the mode is for."""
import numpy as np

EMPTY_REL = 2
ISOLATED = 33
HUB = 5
HUB_EDGES = 300
SIZES = (150, 70)


def empty_tile(n):
    return (64, 128) if n >= 128 else (0, 64)


def edges(n, r, seed=0):
    """-> (src, dst, rel) int64 arrays in shuffled column order"""
    rng = np.random.default_rng(seed + 1000 * n + r)
    lo, hi = empty_tile(n)
    src, dst, rel = [], [], []
    for k in range(r):
        if k == EMPTY_REL:
            continue
        nodes = np.array([i for i in range(n) if i != ISOLATED and not (k == 0 and lo <= i < hi)], dtype=np.int64)
        m = max(4, int(0.7 * nodes.size))               # 1 - exp(-0.7): about half of the segments get an edge
        src.append(rng.choice(nodes, m))
        dst.append(rng.choice(nodes, m))
        rel.append(np.full(m, k, dtype=np.int64))
        if k == 1:                                      # the hub: HUB_EDGES in-edges AND HUB_EDGES out-edges of relation 1
            others = nodes[nodes != HUB]
            src += [rng.choice(others, HUB_EDGES), np.full(HUB_EDGES, HUB, dtype=np.int64)]
            dst += [np.full(HUB_EDGES, HUB, dtype=np.int64), rng.choice(others, HUB_EDGES)]
            rel.append(np.full(2 * HUB_EDGES, k, dtype=np.int64))
    src, dst, rel = (np.concatenate(a) for a in (src, dst, rel))
    order = rng.permutation(src.size)
    return src[order], dst[order], rel[order]


def occupancy(key, rel, n, r):
    """bool [n, r]: segment (key node, relation) has an edge"""
    occ = np.zeros((n, r), dtype=bool)
    occ[key, rel] = True
    return occ


def check_properties(n, r, src, dst, rel):
    """the properties promised above, asserted for both directions"""
    lo, hi = empty_tile(n)
    assert n % 32 and n % 64
    for key in (dst, src):
        occ = occupancy(key, rel, n, r)
        assert not occ[:, EMPTY_REL].any()
        assert not occ[lo:hi, 0].any() and occ[:, 0].any()
        assert not occ[ISOLATED].any()
        assert np.bincount(key * r + rel, minlength=n * r)[HUB * r + 1] > 256
        tile = occ[(HUB // 64) * 64:(HUB // 64) * 64 + 64]
        assert (~tile[:, 1]).any()                      # empty segments of the hub's relation in the hub's tile
        live = occ[:, [k for k in range(r) if k != EMPTY_REL]]
        assert 0.25 < live.mean() < 0.75
