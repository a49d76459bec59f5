"""Writes ``tests/golden/softmax_spread.json``: how far five eager Adam steps of ``train.py --loss softmax`` in float32
on the CPU (the oracle's encoder and the head's torch specification) drift from the same steps in float64 on the same
batches.  ``test_softmax_train.py`` gates the device model at 4 x these figures - same precision, another order of the
N-term sums - and reads them from the file, never from the code under test.  Run on a CPU: ``python
tests/make_softmax_golden.py``.  The model, the graph and the replay live here so that the test uses the same ones."""
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import rgcn_oracle as O                                        # noqa: E402
from primekg_rgcn_linkprediction_amd import head, train as T               # noqa: E402

N, R, EDGES, BATCH, STEPS = 400, 3, 6000, 256, 5
PATH = os.path.join(ROOT, "tests", "golden", "softmax_spread.json")


def graph():
    gen = torch.Generator().manual_seed(3)
    ei, et = torch.randint(0, N, (2, EDGES), generator=gen), torch.randint(0, R, (EDGES,), generator=gen)
    return {"edge_index": ei, "edge_type": et, "num_nodes": N, "num_relations": R}


def arguments(output_dir, device):
    return T.parse_args(["--loss", "softmax", "--dropout", "0", "--decoder_dropout", "0", "--batch_size", str(BATCH),
                         "--filtered_negatives", "--output_dir", str(output_dir), "--device", device])


def initial_state(args):
    """the package's own initialisation (the model's constructor is plain torch)"""
    torch.manual_seed(0)
    return {k: v.clone() for k, v in T.create_model(N, R, args).state_dict().items()}


class _Conv(nn.Module):
    def __init__(self, r, d_in, d_out):
        super().__init__()
        self.weight, self.root = nn.Parameter(torch.zeros(r, d_in, d_out)), nn.Parameter(torch.zeros(d_in, d_out))
        self.bias = nn.Parameter(torch.zeros(d_out))


class _Encoder(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.node_embeddings = nn.Embedding(N, args.embedding_dim)
        self.conv1, self.conv2 = _Conv(R, args.embedding_dim, args.hidden_dim), _Conv(R, args.hidden_dim, args.hidden_dim)

    def forward(self, edge_index, edge_type):
        conv = lambda c: {"weight": c.weight, "root": c.root, "bias": c.bias}        # noqa: E731
        return O.encoder_ref(self.node_embeddings.weight, conv(self.conv1), conv(self.conv2), edge_index, edge_type)


class OracleModel(nn.Module):
    """the model in torch ops under the package's parameter names: the oracle's encoder and, on CPU tensors, the head's
    torch specification of the softmax loss"""

    def __init__(self, args):
        super().__init__()
        self.encoder, self.decoder = _Encoder(args), head.LinkPredictor(R, args.hidden_dim)

    def softmax_loss(self, edge_index, edge_type, heads, tails, rels, **kwargs):
        return self.decoder.softmax_loss(self.encoder(edge_index, edge_type), heads, tails, rels, **kwargs)


def replay(state, batches, args, dtype):
    """the recorded batches through the oracle model in ``dtype``: Adam, clip -> (per-step losses, final parameters)"""
    data = graph()
    model = OracleModel(args).to(dtype)
    model.load_state_dict({k: v.to(dtype) for k, v in state.items()})
    known = T.ops.KnownTriples(data["edge_index"], data["edge_type"], N, R)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    losses = []
    for h, t, r in batches:
        loss, _ = model.softmax_loss(data["edge_index"], data["edge_type"], h, t, r, known=known)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), args.grad_clip)
        opt.step()
        losses.append(loss.item())
    return losses, {k: v.detach().double() for k, v in model.state_dict().items()}


def deviation(losses, params, losses64, params64):
    return {"loss": max(abs(a - b) for a, b in zip(losses, losses64)),
            "params": {k: (params[k].double() - params64[k]).abs().max().item() for k in params64}}


def main():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        args = arguments(tmp, "cpu")
        # the float32 fallback through the trainer itself, on the CPU: its batches are the record (and, the host RNG
        # being where the GPU test's is when its trainer draws the permutation, the batches of that test)
        model = OracleModel(args)
        state = initial_state(args)
        model.load_state_dict(state)
        data = graph()
        trainer = T.Trainer(model, data, data, data, torch.device("cpu"), args)
        log = []
        trainer.train_epoch(on_step=lambda h, t, r, _, loss: log.append((h.clone(), t.clone(), r.clone(), loss.item())),
                            max_steps=STEPS)
        batches = [(h, t, r) for h, t, r, _ in log]
        losses32, params32 = [entry[3] for entry in log], {k: v.detach().double() for k, v in model.state_dict().items()}
        again32, _ = replay(state, batches, args, torch.float32)
        assert max(abs(a - b) for a, b in zip(losses32, again32)) == 0.0, "the replay is not the trainer's step"
        losses64, params64 = replay(state, batches, args, torch.float64)
        spread = deviation(losses32, params32, losses64, params64)
        spread["what"] = ("max |float32 CPU fallback - float64| over %d Adam steps of train.py --loss softmax on the same "
                          "batches: per-step loss, and every parameter afterwards" % STEPS)
        spread["first_batch_heads"] = batches[0][0][:8].tolist()
    with open(PATH, "w") as f:
        json.dump(spread, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(spread, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
