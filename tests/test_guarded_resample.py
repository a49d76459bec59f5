"""The three resampling entry points under the guarded tier's protocol (``test_guarded.protocol``: plain, then every
``ops._empty`` allocation banded and pre-filled with 0x00, then with 0xFF, then with every base moved by 16 bytes): no
band byte changes, no input changes, the same output bits in all four runs - so no output row is written past
``replicates + 1``, no sample is read past ``n`` by the four-at-a-time loads of a ragged last tile, and every output
word that is returned was written.  ``n = T + 1``: a full tile and a tile of one sample, with a tie group laid across
the boundary, so the carried prefix and the carried tie-group start are what the second tile runs on."""
import numpy as np
import pytest
import torch

import resample_reference as R
from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import _lib, ops
from test_guarded import protocol

pytestmark = pytest.mark.gpu

T = _lib.RESAMPLE_TILE
SEED, REPS = (7 << 32) | 99, 6


def test_classification_counts(monkeypatch):
    dev = need_gpu()
    n = T + 1
    assert n > T and n % 4                                   # the carry path, and a ragged quad at the end
    scores = np.arange(n, 0, -1, dtype=np.float64) / 4096.0
    scores[T - 3:T + 1] = scores[T - 3]                      # a tie group over positions T - 3 .. T: across the boundary
    rng = np.random.RandomState(1)
    perm = rng.permutation(n)
    scores, labels = scores[perm], (rng.rand(n) < 0.5).astype(np.int64)
    units = np.arange(n) % ((n + 1) // 2)
    ordered = R.sort_samples(scores, labels, units)
    assert ordered[3][T - 4] and not ordered[3][T - 3:T].any() and ordered[3][T]
    want = [R.curves_sorted(*ordered, 0.125, b, SEED) for b in range(REPS + 1)]
    s, y = torch.as_tensor(scores, dtype=torch.float32).to(dev), torch.as_tensor(labels).to(dev)
    u = torch.as_tensor(units, dtype=torch.int32).to(dev)

    def fn(ctx):
        got = ops.classification_counts(s, y, u, REPS, SEED, 0.125)
        torch.cuda.synchronize()
        for f in ("wp", "wn", "auc2", "tp", "fp"):
            assert getattr(got, f).tolist() == [w[f] for w in want], f
        return list(got)

    protocol(monkeypatch, [s, y, u], fn)


def test_rank_sums(monkeypatch):
    dev = need_gpu()
    m = T + 1
    assert m > T
    rng = np.random.RandomState(2)
    ranks_np, units = rng.randint(1, 5000, m), np.arange(m) % ((m + 1) // 2)
    want = [R.rank_sums(ranks_np, units, (1, 10, 100), b, SEED) for b in range(REPS + 1)]
    ranks, u = torch.as_tensor(ranks_np).to(dev), torch.as_tensor(units, dtype=torch.int32).to(dev)

    def fn(ctx):
        got = ops.rank_sums(ranks, u, (1, 10, 100), REPS, SEED)
        torch.cuda.synchronize()
        assert got.w_sum.tolist() == [w["w_sum"] for w in want] and got.hit_sums.tolist() == [w["hits"] for w in want]
        return list(got[:4])

    protocol(monkeypatch, [ranks, u], fn)


def test_resample_weights(monkeypatch):
    dev = need_gpu()
    units = 257                                              # two workgroups per row, the second with one unit
    want = [R.weights(np.arange(units), b, SEED).tolist() for b in range(REPS + 1)]
    anchor = torch.zeros(1, device=dev)

    def fn(ctx):
        got = ops.resample_weights(units, REPS, SEED, device=dev)
        torch.cuda.synchronize()
        assert got.tolist() == want
        return [got]

    protocol(monkeypatch, [anchor], fn)
