"""Writes ``primekg_node_types.npz``: the node class of every node of the real PrimeKG drug / gene / disease
subgraph (int8 [30926]; class ids by sorted type name) and the class names, read from the reference's
``data/processed/mappings.pt`` (a data file: dicts of str / int / tuple, loaded with ``weights_only=True``).
With ``primekg_test_edges.npz`` it lets a test rank the real test edges type-constrained.

    python tests/golden/make_node_types.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from primekg_rgcn_linkprediction_amd.graphio import node_classes  # noqa: E402


def main(ref: str) -> None:
    maps = torch.load(os.path.join(ref, "data/processed/mappings.pt"), weights_only=True)
    num_nodes = len(maps["node2idx"])
    classes, names = node_classes(maps["idx2node"], num_nodes)
    assert num_nodes == 30926 and len(maps["idx2node"]) == 30968 and len(names) < 128
    np.savez_compressed(os.path.join(HERE, "primekg_node_types.npz"), node_class=classes.numpy().astype(np.int8),
                        class_names=np.array(names), num_nodes=np.int64(num_nodes))
    print(names, np.bincount(classes.numpy()).tolist())


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("RGCN_REFERENCE", "reference"))
