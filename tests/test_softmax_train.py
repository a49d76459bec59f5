"""``train.py --loss softmax`` on the device: five eager Adam steps of the HIP model against the same steps in float64 on
the CPU (the oracle's encoder, the head's torch specification) with the recorded batches.  Per-step loss and parameter
deviation are gated at 4 x the deviation of the float32 CPU fallback from that float64 run on the same batches - same
precision, another order of the N-term sums: that is what the factor is for - measured on the CPU by
``make_softmax_golden.py`` and read from ``golden/softmax_spread.json``, never from the code under test.

The gate is sharp enough to see a 1-ulp ``logf``: with ``lse = m + logf(sum)`` in float32 the parameters were 3 x to 16 x
as far from float64 as the fallback's (every row's ``lse`` off to the same side, so the rows' coefficient sums added up in
the encoder's gradients); with the slices merged and the logarithm taken in float64 they are 1.0 x to 3.8 x."""
import json

import pytest
import torch

import make_softmax_golden as G
from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import train as T

pytestmark = pytest.mark.gpu


def test_five_softmax_steps_match_float64_on_the_same_batches(tmp_path):
    dev = need_gpu()
    with open(G.PATH) as f:
        spread = json.load(f)
    args = G.arguments(tmp_path, "cuda")
    torch.manual_seed(0)
    model = T.create_model(G.N, G.R, args)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    data = G.graph()
    trainer = T.Trainer(model, data, data, data, dev, args)
    assert trainer.softmax and not trainer.use_hip_graph and trainer._sm_known is not None
    log = []
    trainer.train_epoch(on_step=lambda h, t, r, _, loss: log.append((h.cpu(), t.cpu(), r.cpu(), loss.item())),
                        max_steps=G.STEPS)
    assert trainer._graph is None and len(log) == G.STEPS
    assert log[0][0][:8].tolist() == spread["first_batch_heads"]             # the batches the spread was measured on
    losses64, params64 = G.replay(state, [(h, t, r) for h, t, r, _ in log], args, torch.float64)
    got = G.deviation([entry[3] for entry in log], {k: v.detach().cpu() for k, v in trainer.model.state_dict().items()},
                      losses64, params64)
    print("loss deviation %.3e (float32 fallback %.3e)" % (got["loss"], spread["loss"]))
    for k in sorted(got["params"]):
        print("%-40s %.3e (float32 fallback %.3e)" % (k, got["params"][k], spread["params"][k]))
    assert got["loss"] <= 4 * spread["loss"]
    for k, v in got["params"].items():
        assert v <= 4 * spread["params"][k], k
