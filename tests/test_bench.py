"""bench.py: what a plain run prints and what ``--dump-outputs`` writes (the files that let two builds of the project be
compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, need_gpu
from oracle import rgcn_oracle as O
from primekg_rgcn_linkprediction_amd import RGCNConv, synth

import bench

CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _fake_run(n, d_out, d_in, seed):
    """a bench.Run as far as dump_outputs reads one: two layers' parameters with gradients, an eager last step"""
    gen = torch.Generator().manual_seed(seed)
    run = bench.Run.__new__(bench.Run)
    run.world, run.n = 1, n
    run.convs = [RGCNConv(d_in, 8, 3), RGCNConv(8, d_out, 3)]
    emb = torch.zeros(n, d_in, requires_grad=True)
    run.params = [emb] + [p for c in run.convs for p in c.parameters()]
    for p in run.params:
        p.grad = torch.randn(p.shape, generator=gen)
    out = torch.randn(n, d_out, generator=gen)
    run.last_step = ("eager", out)
    return run, out


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_writes_every_array_whole_when_they_fit(tmp_path):
    run, out = _fake_run(1000, 16, 4, seed=1)
    bench.dump_outputs(run, str(tmp_path), rank=0)
    got = _load(tmp_path)
    assert set(got) == {"encoder_out", "grad_node_embeddings", "grad_conv1_weight", "grad_conv1_root", "grad_conv1_bias",
                        "grad_conv2_weight", "grad_conv2_root", "grad_conv2_bias"}
    assert all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["encoder_out"], out.numpy())
    assert np.array_equal(got["grad_node_embeddings"], run.params[0].grad.numpy())
    assert np.array_equal(got["grad_conv2_weight"], run.convs[1].weight.grad.numpy())


def test_dump_outputs_samples_the_same_node_rows_within_64_mb(tmp_path):
    """[nodes, d] arrays beyond 64 MB in all: one fixed, seeded sample of rows, the same for every such array and every
    run; the parameter gradients stay whole"""
    n = 120_000                                    # (128 + 64) floats per node: 92 MB
    run, out = _fake_run(n, 128, 64, seed=2)
    bench.dump_outputs(run, str(tmp_path / "a"), rank=0)
    bench.dump_outputs(run, str(tmp_path / "b"), rank=0)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 2 ** 20
    rows = a["rows"]
    assert rows.dtype == np.float64 and np.array_equal(rows, b["rows"])
    idx = rows.astype(np.int64)
    assert np.array_equal(idx, rows) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert len(idx) > n // 2
    assert np.array_equal(a["encoder_out"], out.numpy()[idx])
    assert np.array_equal(a["grad_node_embeddings"], run.params[0].grad.numpy()[idx])
    assert np.array_equal(a["grad_conv1_weight"], run.convs[0].weight.grad.numpy())


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_what_its_last_step_computed(tmp_path):
    """``bench.py --gpus 1 --steps 3 --warmup 2 --dump-outputs DIR``: one JSON line with the contract's fields and none
    of the --full legs; the encoder output and conv2's parameter gradients in DIR are within the north-star gates
    (1e-5; 1e-4 of the largest entry) of the float64 evaluation on the same seeded inputs.  The gradients behind the
    ReLU are the parity suite's: they need the device's ReLU decisions, which the files do not carry."""
    need_gpu()
    dump = tmp_path / "outputs"
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                           "--dump-outputs", str(dump)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert all(k in line for k in CONTRACT)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    assert line["value"] == pytest.approx(2 * synth.PRIMEKG_EDGES / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert not {"roofline", "dominant_kernel", "cpu_baseline", "secondary", "fp32_mfma", "drop_in"} & set(line)
    got = _load(dump)
    assert sum(os.path.getsize(dump / f) for f in os.listdir(dump)) <= 64 * 2 ** 20
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())

    # bench.Run's inputs, in its order: graph (seed 42), then under seed 0 the table, both layers and the cotangent
    ei, et, n, r = synth.primekg_like(seed=42)
    torch.manual_seed(0)
    emb = torch.nn.init.xavier_uniform_(torch.empty(n, 64))
    convs = [RGCNConv(64, 128, r), RGCNConv(128, 128, r)]
    cot = torch.randn(n, 128)
    f64 = O.encoder_explicit_f64(emb, *[{k: v.detach() for k, v in c.named_parameters()} for c in convs], ei, et, cot)
    assert got["encoder_out"].shape == (n, 128) and got["grad_node_embeddings"].shape == (n, 64)
    assert np.abs(got["encoder_out"] - f64["out"].numpy()).max() <= 1e-5
    for k, _ in convs[1].named_parameters():
        g = f64["grads"][f"conv2.{k}"].numpy()
        assert np.abs(got[f"grad_conv2_{k}"] - g).max() <= 1e-4 * np.abs(g).max(), k
