"""Host tier (no GPU): the occupancy order of a structure's rows (``include/rgcn_row_order.h``) - what the graph builders
upload behind the occupancy words, computed by the library's own host routine from ``rowptr`` and held to its
definition: a permutation of the rows, grouped by occupancy word, heavier words first, natural order inside a group;
the row and tile words in that order; the deferred hub items regrouped by the tile that holds their destination - and
the places the mode's option bit and its policy switch are written down."""
import ctypes
import os
import re

import numpy as np
import pytest

import c_surface as S
from primekg_rgcn_linkprediction_amd import _lib, conv

PACK_SPAN = 256                                        # RGCN_CHUNK * RGCN_PACK: longer segments leave partial rows


def _rowptr(key, rel, n, r):
    counts = np.bincount(key * r + rel, minlength=n * r)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _graph(n, r, seed, hubs=()):
    """(key, rel) of a typed graph whose occupancy is scattered: row i has the relations of word (5 i + 3) mod 2^r (every
    word occurs once n >= 2^r, the empty one - rows without any edge - included), the last relation has no edge at all
    when `r` > 3, and segment (row, relation) of each entry of `hubs` has that many edges"""
    rng = np.random.default_rng(seed)
    live = r - 1 if r > 3 else r
    key, rel = [], []
    for i in range(n):
        word = (5 * i + 3) % (1 << live)
        for b in range(live):
            if word >> b & 1:
                k = int(rng.integers(1, 4))
                key += [i] * k
                rel += [b] * k
    for (row, b, count) in hubs:
        key += [row] * count
        rel += [b] * count
    return np.array(key, dtype=np.int64), np.array(rel, dtype=np.int64)


def _order(rowptr, n, r):
    lib = _lib.load()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    lay = _lib.RowOrderLayout()
    total = lib.rgcn_row_order_host(rp.ctypes.data, n, r, None, ctypes.byref(lay))
    assert total > 0 and total == lay.total_words
    words = np.full(total, 0xDEADBEEF, dtype=np.uint32)
    again = _lib.RowOrderLayout()
    assert lib.rgcn_row_order_host(rp.ctypes.data, n, r, words.ctypes.data, ctypes.byref(again)) == total
    assert all(getattr(lay, f) == getattr(again, f) for f, _ in _lib.RowOrderLayout._fields_)
    return words, lay


def _popcount(a):
    return np.array([bin(int(v)).count("1") for v in a], dtype=np.int64)


CASES = [(40, 3, ()), (130, 3, ()), (193, 3, ()), (64, 3, ()), (128, 3, ()), (7, 3, ()), (50, 1, ()), (97, 5, ()),
         (150, 3, ((3, 0, 300), (77, 2, 600))), (33, 32, ())]


@pytest.mark.parametrize("n,r,hubs", CASES)
def test_the_order_is_what_the_header_says(n, r, hubs):
    lib = _lib.load()
    for transposed in (False, True):                   # two different structures over the same rows
        key, rel = _graph(n, r, 100 * n + r + transposed, hubs)
        if transposed:
            key = (key * 7 + 1) % n
        rowptr = _rowptr(key, rel, n, r)
        words, lay = _order(rowptr, n, r)
        # the natural-order words in front are what rgcn_occupancy_host gives, untouched
        off = ctypes.c_int64(-1)
        occ_total = lib.rgcn_occupancy_host(None, n, r, None, ctypes.byref(off))
        occ = np.zeros(occ_total, dtype=np.uint32)
        assert lib.rgcn_occupancy_host(rowptr.ctypes.data, n, r, occ.ctypes.data, None) == occ_total
        assert np.array_equal(words[:occ_total], occ)
        rows = occ[off.value:off.value + n]
        if n >= 8 and r == 3 and not transposed:
            assert set(rows.tolist()) == set(range(8))  # all eight occupancy words, rows without any edge among them
        # layout: P, sections in order, each on a 16-byte boundary, nothing between the pad words and the order but zeros
        p = lay.padded_rows
        assert p == (n + 63) // 64 * 64
        assert lay.perm == (occ_total + 3) // 4 * 4 and lay.row_words == lay.perm + p and lay.tile_words == lay.row_words + p
        assert lay.fin_ptr >= lay.tile_words + p // 32 and lay.items >= lay.fin_ptr + p // 32 + 1
        assert all(o % 4 == 0 for o in (lay.perm, lay.row_words, lay.tile_words, lay.fin_ptr, lay.items))
        assert lay.total_words == lay.items + 4 * lay.num_items
        assert not words[occ_total:lay.perm].any()
        perm = words[lay.perm:lay.perm + p].astype(np.int64)
        # a permutation of the rows; positions past n hold a valid row
        assert np.array_equal(np.sort(perm[:n]), np.arange(n)) and (perm[n:] < n).all()
        # the row words in that order (0 past n) and every tile word the OR of its rows' words
        rw = words[lay.row_words:lay.row_words + p]
        assert np.array_equal(rw[:n], rows[perm[:n]]) and not rw[n:].any()
        tw = words[lay.tile_words:lay.tile_words + p // 32]
        assert np.array_equal(tw, np.bitwise_or.reduce(rw.reshape(-1, 32), axis=1))
        assert not words[lay.tile_words + p // 32:lay.fin_ptr].any()
        # groups are contiguous, heavier words first, natural order inside a group
        change = np.flatnonzero(np.diff(rw[:n].astype(np.int64)) != 0) + 1
        starts = np.concatenate([[0], change])
        group_words = rw[:n][starts]
        assert len(set(group_words.tolist())) == len(group_words)
        pc = _popcount(group_words)
        assert (np.diff(pc) <= 0).all()
        same = np.diff(pc) == 0
        assert (np.diff(group_words.astype(np.int64))[same] > 0).all()
        for b, e in zip(starts, np.concatenate([change, [n]])):
            assert (np.diff(perm[b:e]) > 0).all()
        # deferred hub items: every one once, under the 32-position tile that holds its destination row
        seg_len = np.diff(rowptr.astype(np.int64))
        hub_segs = np.flatnonzero(seg_len > PACK_SPAN)
        assert lay.num_items == len(hub_segs) == (len(hubs) if hubs else 0)
        fin = words[lay.fin_ptr:lay.fin_ptr + p // 32 + 1].astype(np.int64)
        assert fin[0] == 0 and fin[-1] == lay.num_items and (np.diff(fin) >= 0).all()
        if lay.num_items:
            items = words[lay.items:lay.items + 4 * lay.num_items].astype(np.int64).reshape(-1, 4)
            assert sorted(items[:, 2].tolist()) == hub_segs.tolist()          # dst: each hub segment exactly once
            assert (items[:, 3] & 1).all()                                    # RGCN_ITEM_FINAL
            assert np.array_equal(items[:, 1] - items[:, 0], -(-seg_len[items[:, 2]] // PACK_SPAN))
            spans = sorted(map(tuple, items[:, :2].tolist()))                 # their partial rows tile [0, num_partials)
            assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            pos = np.empty(n, dtype=np.int64)
            pos[perm[:n]] = np.arange(n)
            for t in range(p // 32):
                for j in range(fin[t], fin[t + 1]):
                    assert pos[items[j, 2] // r] >> 5 == t


def test_sorted_tiles_are_not_mixed_where_natural_tiles_are():
    n, r = 193, 3
    key, rel = _graph(n, r, 1)
    rowptr = _rowptr(key, rel, n, r)
    words, lay = _order(rowptr, n, r)
    natural = words[:n // 32]                                        # the full natural tiles: each has every relation
    ordered = words[lay.tile_words:lay.tile_words + lay.padded_rows // 32]
    assert _popcount(natural).sum() == 3 * len(natural)
    # (eight words of 24 rows each against 32-row tiles: 14 live (tile, relation) blocks where node order has 18 + 2)
    assert _popcount(ordered).sum() <= 0.75 * _popcount(words[:(n + 31) // 32]).sum()


def test_structures_without_an_order_and_bad_arguments():
    lib = _lib.load()
    lay = _lib.RowOrderLayout()
    rowptr = np.zeros(40 * 33 + 1, dtype=np.int32)
    assert lib.rgcn_row_order_host(rowptr.ctypes.data, 40, 33, None, ctypes.byref(lay)) == 0 and lay.total_words == 0
    assert lib.rgcn_row_order_host(rowptr.ctypes.data, 0, 3, None, None) == 0
    assert lib.rgcn_row_order_host(None, 4, 3, None, None) < 0
    assert lib.rgcn_row_order_host(rowptr.ctypes.data, -1, 3, None, None) < 0
    assert lib.rgcn_row_order_host(rowptr.ctypes.data, 4, 0, None, None) < 0
    count = ctypes.c_int64(7)
    assert lib.rgcn_graph_row_order(None, 0, ctypes.byref(count)) is None and count.value == 0


def test_the_header_the_binding_and_the_policy_agree():
    """(the header's functions against the binding and the library: test_c_surface.py, for every header)"""
    text, code = S.header_text("rgcn_row_order.h"), S.header_code("rgcn_row_order.h")
    assert f"#define RGCN_MODE_ROW_ORDER {_lib.MODE_ROW_ORDER}\n" in text
    assert _lib.MODE_ROW_ORDER == 4 and not _lib.MODE_ROW_ORDER & (1 | _lib.MODE_SPARSE_ROWS)
    fields = re.search(r"typedef struct rgcn_row_order_layout \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", fields) == [f for f, _ in _lib.RowOrderLayout._fields_]
    # the switch is a module attribute that recorded passes are keyed by, like _SPARSE_AGG; on unless the environment says 0
    assert conv._NT_ROW_ORDER is (os.environ.get("RGCN_NT_ROW_ORDER", "1") != "0")
    before = conv._policy_key()
    saved = conv._NT_ROW_ORDER
    conv._NT_ROW_ORDER = not saved
    try:
        assert conv._policy_key() != before
    finally:
        conv._NT_ROW_ORDER = saved
