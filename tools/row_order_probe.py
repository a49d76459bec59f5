"""Probe, before any kernel change: what would the three `k_gemm_nt_split` launches of the C2 step gain if their 64-row
tiles held rows of one occupancy word?  The C2 graph with its NODE IDS RELABELLED so that the natural 64-row tiles are
the tiles an occupancy order would form (features and cotangent permuted to match; the weights do not depend on node
ids), run under rocprofv3 beside the unrelabelled graph.  The graph is symmetric (every pair is two reverse columns),
so one labelling sorts the forward and the transposed structure alike.  The gathers' times under a relabelling are not
the quantity of interest - the real change would move no row - only the NT averages are.

Labellings (484 tiles, the last one partial and left in place):
    natural   the graph as bench.py builds it
    sorted    rows grouped by occupancy word, heavier words (more relations) first, natural order inside a group
    parity    the sorted tiles dealt heavy / light by blockIdx parity (tiles b and b + 1 are a heavy and a light one)
    pair256   the sorted tiles placed so that tiles i and i + 256 are a heavy and a light one

    python3 tools/row_order_probe.py stats                         (CPU: live k-tiles per workgroup under each labelling)
    python3 tools/row_order_probe.py masks DIR && tools/gemm_stamps DIR/*.u32   (the NT forward launch alone, per labelling)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python3 tools/row_order_probe.py run LABELLING
    python3 tools/row_order_probe.py table NAME=kernel_stats.csv ...   (the table of profiles/nt_row_order.txt)
"""
import csv
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE = 64
LABELLINGS = ("natural", "sorted", "parity", "pair256")
STEP_KERNELS = ("k_gemm_nt_split", "k_gemm_tn_coop", "k_aggregate", "k_absmax_pack", "k_absmax_multi", "k_reduce_partials")


def occupancy_words(ei, et, n):
    """int64 [n]: bit r set where node i has an incoming edge of relation r (the row word of the forward structure;
    the transposed structure's is the same on a symmetric graph)"""
    words = torch.zeros(n, dtype=torch.int64)
    for r in range(int(et.max()) + 1):
        has = torch.zeros(n, dtype=torch.bool)
        has[ei[1, et == r]] = True
        words |= has.to(torch.int64) << r
    return words


def popcount(words):
    return sum((words >> b) & 1 for b in range(32))


def order_of(words, labelling):
    """int64 [n]: order[i] = the old id of the node that gets id i"""
    n = words.numel()
    if labelling == "natural":
        return torch.arange(n)
    # heavier groups first, groups by word, natural order inside a group (stable sort on one key)
    key = (32 - popcount(words)) * (1 << 32) + words
    order = torch.sort(key, stable=True).indices
    full = n // TILE                                     # full tiles; a partial last tile keeps its place
    if labelling == "sorted":
        return order
    tiles = order[:full * TILE].view(full, TILE)         # tile 0 heaviest ... tile full - 1 lightest
    if labelling == "parity":
        src = [p // 2 if p % 2 == 0 else full - 1 - p // 2 for p in range(full)]
    elif labelling == "pair256":
        first = min(256, full)
        src = list(range(first)) + [full - 1 - i for i in range(full - first)]
    else:
        raise SystemExit(f"unknown labelling {labelling!r}: one of {LABELLINGS}")
    assert sorted(src) == list(range(full))
    return torch.cat([tiles[torch.tensor(src)].reshape(-1), order[full * TILE:]])


def relabel(ei, order):
    new_id = torch.empty_like(order)
    new_id[order] = torch.arange(order.numel())
    return new_id[ei]


def live_ktiles(words, order, r, d_in):
    """per 64-row tile of the labelling: live 32-wide k-tiles of [agg | x] (a relation's d_in / 32 k-tiles are live
    where any row of the tile has the relation; the root block is always live)"""
    w = words[order]
    pad = (-w.numel()) % TILE
    w = torch.cat([w, torch.zeros(pad, dtype=torch.int64)]).view(-1, TILE)
    tile_word = torch.zeros(w.size(0), dtype=torch.int64)
    for j in range(TILE):
        tile_word |= w[:, j]
    return (popcount(tile_word) + 1) * (d_in // 32)


def stats():
    from primekg_rgcn_linkprediction_amd import synth
    ei, et, n, r = synth.primekg_like()
    words = occupancy_words(ei, et, n)
    tiles = (n + TILE - 1) // TILE
    print(f"C2: {n} rows, {r} relations, {tiles} tiles of {TILE} rows; "
          f"(row, relation) segments with an edge: {float(popcount(words).sum()) / (n * r):.3f}")
    print("labelling   live k-tiles per workgroup, mean (max) at K = 512 / K = 256    worst of (b, b+1) / (b, b+256) pair sums at K = 512")
    for lab in LABELLINGS:
        order = order_of(words, lab)
        assert torch.equal(torch.sort(order).values, torch.arange(n))
        k512, k256 = live_ktiles(words, order, r, 128), live_ktiles(words, order, r, 64)
        even = k512[0:tiles - tiles % 2:2] + k512[1::2]
        far = k512[:tiles - 256] + k512[256:]
        print(f"{lab:10s}  {float(k512.float().mean()):5.2f} ({int(k512.max())}) / {float(k256.float().mean()):5.2f} ({int(k256.max())})"
              f"{'':36s}{int(even.max())} / {int(far.max())}")


def masks(outdir):
    """OUTDIR/<labelling>.u32: the relation word of every 32-row tile under each labelling, the `tile_mask` operand of
    the NT kernels - `tools/gemm_stamps OUTDIR/*.u32` times the NT forward launch alone under each of them"""
    import numpy as np
    from primekg_rgcn_linkprediction_amd import synth
    ei, et, n, _ = synth.primekg_like()
    words = occupancy_words(ei, et, n)
    os.makedirs(outdir, exist_ok=True)
    for lab in LABELLINGS:
        w = words[order_of(words, lab)]
        w = torch.cat([w, torch.zeros((-n) % 32, dtype=torch.int64)]).view(-1, 32)
        tile_word = torch.zeros(w.size(0), dtype=torch.int64)
        for j in range(32):
            tile_word |= w[:, j]
        tile_word.numpy().astype(np.uint32).tofile(os.path.join(outdir, f"{lab}.u32"))


def run(labelling, steps=300):
    """the bench step (bench.py's `Run.step`, eager) on the relabelled graph; rocprofv3 wraps this process"""
    from primekg_rgcn_linkprediction_amd import RGCNConv, rgcn_encoder2, synth
    dev = torch.device("cuda:0")
    ei, et, n, r = synth.primekg_like(seed=42)
    order = order_of(occupancy_words(ei, et, n), labelling)
    eid, etd = relabel(ei, order).to(dev), et.to(dev)
    torch.manual_seed(0)
    emb = torch.nn.init.xavier_uniform_(torch.empty(n, 64))[order].to(dev).requires_grad_(True)
    convs = [RGCNConv(64, 128, r).to(dev), RGCNConv(128, 128, r).to(dev)]
    cot = torch.randn(n, 128)[order].to(dev)
    params = [emb] + [p for c in convs for p in c.parameters()]
    for _ in range(steps):
        out = rgcn_encoder2(emb, eid, etd, convs[0], convs[1])
        for p in params:
            p.grad = None
        out.backward(cot)
    torch.cuda.synchronize()
    print(f"{labelling}: {steps} steps done")


def short(name):
    """`k_gemm_nt_split<2, 2, 2, 1, true, false>` from a rocprofv3 kernel name"""
    name = name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
    # an instantiation with the ORDER argument stands beside the one without it
    return re.sub(r"^(k_gemm_nt_split<(?:[^,>]+, ){5}[^,>]+), (?:true|false)>$", r"\1>", name)


def table(pairs):
    cols = []
    for pair in pairs:
        label, path = pair.split("=", 1)
        per = {}
        for row in csv.DictReader(open(path)):
            k = short(row["Name"])
            if k.startswith(STEP_KERNELS) and int(row["Calls"]) >= 100:
                per[k] = float(row["AverageNs"]) * 1e-3
        cols.append((label, per))
    kernels = sorted({k for _, per in cols for k in per}, key=lambda k: (not k.startswith("k_gemm_nt"), k))
    print("rocprofv3 --kernel-trace --stats, average us per launch" + "".join(f"{label:>11s}" for label, _ in cols))
    for k in kernels:
        print(f"{k:55s}" + "".join(f"{per.get(k, float('nan')):11.2f}" for _, per in cols))
    for what, pick in (("sum of the three k_gemm_nt_split", lambda k: k.startswith("k_gemm_nt")), ("sum of all listed", lambda k: True)):
        print(f"{what:55s}" + "".join(f"{sum(v for k, v in per.items() if pick(k)):11.2f}" for _, per in cols))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "stats"
    if mode == "stats":
        stats()
    elif mode == "masks":
        masks(sys.argv[2])
    elif mode == "run":
        run(sys.argv[2])
    elif mode == "table":
        table(sys.argv[2:])
    else:
        raise SystemExit(__doc__)
