"""Host tier (no GPU): the row-granular occupancy a sparse aggregate rests on (``include/rgcn_sparse.h``) - the words
the graph builders upload, computed by the library's own host routine and held to a NumPy restatement from ``rowptr`` -
and the places the mode's one option bit and its policy switch are written down."""
import ctypes

import numpy as np
import pytest

import c_surface as S
import sparse_graphs as SG
from primekg_rgcn_linkprediction_amd import _lib, conv

PAD = 96                                                # RGCN_ROW_MASK_PAD


def _rowptr(key, rel, n, r):
    counts = np.bincount(key * r + rel, minlength=n * r)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _host_words(rowptr, n, r):
    lib = _lib.load()
    off = ctypes.c_int64(-1)
    total = lib.rgcn_occupancy_host(None, n, r, None, ctypes.byref(off))
    if total <= 0:
        return total, off.value, None
    words = np.full(total, 0xDEADBEEF, dtype=np.uint32)
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    got = lib.rgcn_occupancy_host(rp.ctypes.data, n, r, words.ctypes.data, None)
    assert got == total
    return total, off.value, words


def _expected_rows(rowptr, n, r):
    live = (np.diff(rowptr.astype(np.int64)) > 0).reshape(n, r)
    return (live.astype(np.uint64) << np.arange(r, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


@pytest.mark.parametrize("n", SG.SIZES)
@pytest.mark.parametrize("r", [3, 5])
def test_the_test_graphs_have_the_properties_they_promise(n, r):
    SG.check_properties(n, r, *SG.edges(n, r))


@pytest.mark.parametrize("n,r", [(150, 3), (70, 5), (64, 3), (33, 32), (1, 1)])
def test_row_words_are_the_segment_occupancy_and_tile_words_their_or(n, r):
    if r in (3, 5) and n in SG.SIZES:
        src, dst, rel = SG.edges(n, r)
    else:
        rng = np.random.default_rng(n * 100 + r)
        e = 2 * n
        src, dst, rel = rng.integers(0, n, e), rng.integers(0, n, e), rng.integers(0, r, e)
        rel[: min(e, r)] = np.arange(min(e, r))          # every relation bit, the top one (bit 31) included
    for key in (dst, src):                               # the forward and the transposed structure
        rowptr = _rowptr(key, rel, n, r)
        total, off, words = _host_words(rowptr, n, r)
        tiles = (n + 31) // 32
        assert off == (tiles + 3) // 4 * 4 and total == off + n + PAD
        rows = _expected_rows(rowptr, n, r)
        assert np.array_equal(words[off:off + n], rows)
        assert np.array_equal(rows != 0, SG.occupancy(key, rel, n, r).any(axis=1))
        padded = np.zeros(tiles * 32, dtype=np.uint32)
        padded[:n] = rows
        assert np.array_equal(words[:tiles], np.bitwise_or.reduce(padded.reshape(tiles, 32), axis=1))
        assert not words[tiles:off].any() and not words[off + n:].any()      # alignment gap and the tail: zeros
    if r == 32:
        assert (words[off:off + n] >> 31).any()


def test_more_than_32_relations_have_no_occupancy_words():
    n, r = 40, 33
    rowptr = np.zeros(n * r + 1, dtype=np.int32)
    total, off, words = _host_words(rowptr, n, r)
    assert total == 0 and words is None and off == 4     # nothing to write; the consumers then read every row
    lib = _lib.load()
    assert lib.rgcn_occupancy_host(None, -1, 3, None, None) < 0 and lib.rgcn_occupancy_host(None, 4, 0, None, None) < 0
    count = ctypes.c_int64(7)
    assert lib.rgcn_graph_row_mask(None, 0, ctypes.byref(count)) is None and count.value == 0


def test_the_header_the_binding_and_the_policy_agree():
    """(the header against the binding and the library: test_c_surface.py, for every header)"""
    main = S.header_text("rgcn_hip.h")
    assert f"#define RGCN_MODE_SPARSE_ROWS {_lib.MODE_SPARSE_ROWS}\n" in main and _lib.MODE_SPARSE_ROWS == 2
    # the switch is a module attribute that recorded passes are keyed by, like _DEFER_HUBS
    assert conv._SPARSE_AGG is True and conv._SPARSE_AGG in conv._policy_key()
    before = conv._policy_key()
    conv._SPARSE_AGG = False
    try:
        assert conv._policy_key() != before
    finally:
        conv._SPARSE_AGG = True
