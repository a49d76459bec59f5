"""The t-SNE entry points under the guarded tier's protocol (``test_guarded.protocol``: plain, then every ``ops._empty``
allocation banded and pre-filled with 0x00, then with 0xFF): no band byte changes, no input changes, the same output bits
in all three runs.  M = 257 (one row past a 256-row tile: two row tiles, two column tiles), d = 32, k = 64 (one candidate
past a wave: both candidate slots of a lane are in use)."""
import pytest
import torch

import tsne_reference as R
from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import _lib, ops
from test_guarded import protocol

pytestmark = pytest.mark.gpu

M, D, K = 257, 32, 64


def _rows(dev):
    return torch.from_numpy(R.blobs(M, D, seed=257)).float().to(dev)


def test_knn(monkeypatch):
    dev = need_gpu()
    x = _rows(dev)
    assert K + 1 > 64 and K + 1 <= ops.TOPK_MAX_K and M > 256            # the second candidate slot; a partial last workgroup
    protocol(monkeypatch, [x], lambda ctx: list(ops.knn(x, K)))


def test_affinities_and_joint(monkeypatch):
    dev = need_gpu()
    ids, sqdist = ops.knn(_rows(dev), K)
    assert sqdist.shape == (M, K) and K > 64 - 1 and M % 4 == 1            # lanes 0 .. 63 hold a first neighbour; a partial workgroup

    def fn(ctx):
        cond_p, beta = ops.tsne_affinities(sqdist, 30.0)
        return [cond_p, beta] + list(ops.tsne_joint(ids, cond_p))

    protocol(monkeypatch, [ids, sqdist], fn)


def test_gradient_and_update(monkeypatch):
    dev = need_gpu()
    ids, sqdist = ops.knn(_rows(dev), K)
    rowptr, col, val = ops.tsne_joint(ids, ops.tsne_affinities(sqdist, 30.0)[0])
    gen = torch.Generator().manual_seed(5)
    y0, upd0 = torch.randn(M, 2, generator=gen).to(dev), (torch.randn(M, 2, generator=gen) * 0.1).to(dev)
    gains0 = (torch.rand(M, 2, generator=gen) * 2 + 0.005).to(dev)
    size = _lib.load().rgcn_tsne_workspace_bytes
    assert size(M, 2) > size(M, 1) and size(M, 2) == size(M, 7)          # two column tiles: two slices are really used

    def fn(ctx):
        y, update, gains = ctx.like(y0), ctx.like(upd0), ctx.like(gains0)
        grad, z, kl = ops.tsne_gradient(y, rowptr, col, val, exaggeration=12.0, slices=2, compute_error=True)
        norm2 = ops.tsne_update(grad, y, update, gains, 0.5, 50.0)
        quiet = ops.tsne_gradient(y, rowptr, col, val, exaggeration=1.0, slices=2, compute_error=False)
        return [grad, z, kl, norm2, y, update, gains, list(quiet)]

    protocol(monkeypatch, [y0, upd0, gains0, rowptr, col, val], fn)
