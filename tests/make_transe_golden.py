"""Writes ``tests/golden/transe_spread.json``: the seed spread of the reference's TransE, against which the device fit is
judged (``tests/test_transe.py``) - a fit in the reference's sample order (``transe_reference.fit(order="sample")``,
numpy float64) on ``transe_reference.zipf_graph()`` per seed, its last-epoch mean loss and the share of the columns whose
positive lies closer than a fresh corruption.  A few seconds of numpy:

    python tests/make_transe_golden.py
"""
import json
import os

import transe_reference as R

CONFIG = {"num_nodes": 1500, "num_edges": 12000, "num_relations": 3, "graph_seed": 0, "exponent": 0.9,
          "d": 64, "epochs": 4, "batch": 1024, "lr": 0.01, "margin": 1.0}
SEEDS = list(range(8))


def one_seed(seed, config=CONFIG):
    ei, et = R.zipf_graph(config["num_nodes"], config["num_edges"], config["num_relations"], config["graph_seed"],
                          config["exponent"])
    e, r, loss = R.fit(ei, et, config["num_nodes"], config["num_relations"], config["d"], config["epochs"], config["batch"],
                       config["lr"], config["margin"], seed, order="sample")
    return {"loss": loss, "closer_share": R.closer_share(e, r, ei, et, seed)}


if __name__ == "__main__":
    out = {"config": CONFIG, "order": "sample", "seeds": {str(s): one_seed(s) for s in SEEDS}}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transe_spread.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out["seeds"], indent=1))
