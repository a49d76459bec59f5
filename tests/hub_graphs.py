"""Graphs whose hub segments need a THIRD level of the gather's plan (``csrc/rgcn_plan.h``: runs of 64 edges, four
runs to a pack, reduce levels of fan-in 512 - a third level past 64 * 4 * 512 = 131,072 edges in one (node, relation)
segment), shared by ``test_hub_levels.py`` and the guarded family of ``test_guarded.py``, and the exact expectations
of gathers over them: with few nodes a segment sum is ``counts[segment, source] @ table`` in int64."""
import torch

N, R = 64, 2
# (node, relation) of the three hubs: the largest two-level segment sits in the second block of 32 rows, the smallest
# three-level one (its last pack holds ONE edge, its second level-1 item ONE row) and one whose level-1 items hold
# 512, 512 and 5 rows in the first
HUBS = {(40, 0): 131072, (3, 0): 131073, (5, 1): 262444}
# the lengths of test_segment_lengths_around_run_and_pack_boundaries, some of them twice: forty short segments
SHORT = [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 511, 512, 513,
         1023, 1024, 1025, 2049, 16385 + 3 * 256 + 70]
SHORT = SHORT + SHORT[3:17]


def segment_lengths():
    """length of every (node, relation) segment of the boundary graph, ``[N * R]``"""
    lens = torch.zeros(N * R, dtype=torch.int64)
    for (node, rel), length in HUBS.items():
        lens[node * R + rel] = length
    free = [s for s in range(N * R) if lens[s] == 0]
    for i, length in enumerate(SHORT):
        lens[free[3 * i + 1]] = length                      # spread over both blocks of 32 rows and both relations
    return lens


def boundary_edges(seed=0):
    """``(key, other, rel)`` int64[E] in shuffled column order: ``key`` owns the segments above, ``other`` is random"""
    gen = torch.Generator().manual_seed(seed)
    lens = segment_lengths()
    seg = torch.repeat_interleave(torch.arange(N * R), lens)
    other = torch.randint(0, N, (seg.numel(),), generator=gen)
    order = torch.randperm(seg.numel(), generator=gen)
    return (seg // R)[order].contiguous(), other[order].contiguous(), (seg % R)[order].contiguous()


def plan_partials(lens):
    """rows of partial-sum workspace the plan needs for segments of these lengths, restated from the constants: one row
    per pack of 256 edges when there is more than one pack, then one row per run of 512 rows until one run is left"""
    total = 0
    for length in lens.tolist():
        rows = -(-length // 256)
        while rows > 1:
            total += rows
            rows = -(-rows // 512) if rows > 512 else 1
    return total


def plan_levels(lens):
    deepest = 1
    for length in lens.tolist():
        rows, levels = -(-length // 256), 1
        while rows > 1:
            levels += 1
            rows = -(-rows // 512) if rows > 512 else 1
        deepest = max(deepest, levels)
    return deepest


def segment_matrix(key, other, rel, weight=None):
    """int64 ``[N * R, N]``: per (segment, other node) the number of edges, or the sum of their integer weights"""
    flat = (key * R + rel) * N + other
    ones = torch.ones_like(flat) if weight is None else weight
    return torch.zeros(N * R * N, dtype=torch.int64).index_add_(0, flat, ones).view(N * R, N)


def int_table(d, bound, seed):
    return torch.randint(-bound, bound + 1, (N, d), generator=torch.Generator().manual_seed(seed))


def mean_expected(key, other, rel, table):
    """the int64 segment sums of an integer ``table``, cast to fp32 (exact below 2^24) and divided in fp32 by
    ``max(1, len)`` -> ``[N, R * d]``"""
    sums = segment_matrix(key, other, rel) @ table.long()
    cnt = torch.bincount(key * R + rel, minlength=N * R).clamp(min=1)
    return (sums.float() / cnt.float().view(-1, 1)).view(N, -1)
