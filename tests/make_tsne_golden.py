"""Writes ``tests/golden/tsne_blobs300.json``: what a whole t-SNE run reaches on one small input, by four CPU runs.

Setting: ``blobs(300, 32, seed=11)``, perplexity 30, PCA init, 500 iterations.  Recorded: the final KL divergence and the
trustworthiness (10 neighbours) of the float64 restatement (``tsne_reference.run``), its float32 variant, scikit-learn's
``TSNE(angle=0.0)`` and ``TSNE(angle=0.5)``, all from that init; and the same two figures of a seeded random layout of the
float64 run's spread.  A trajectory amplifies rounding, so the four runs end in different layouts: their spread is what
the GPU tier's whole-run gates are made of.  Needs scikit-learn; run from the repository root:

    python tests/make_tsne_golden.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsne_reference as R  # noqa: E402

SETTING = {"m": 300, "d": 32, "seed": 11, "perplexity": 30.0, "max_iter": 500, "trust_neighbors": 10, "init": "pca"}


def main():
    from sklearn.manifold import TSNE
    s = SETTING
    x = R.blobs(s["m"], s["d"], seed=s["seed"])
    p = R.affinities(x, s["perplexity"])
    y0 = R.pca_init(x)
    runs = {}
    layouts = {}
    for name, dtype in (("restatement_float64", np.float64), ("restatement_float32", np.float32)):
        y, kl, n_iter = R.run(p, y0, s["max_iter"], dtype=dtype)
        assert n_iter == s["max_iter"]
        layouts[name] = y
        runs[name] = {"kl": float(kl), "trustworthiness": float(R.trustworthiness(x, y, s["trust_neighbors"]))}
    for angle in (0.0, 0.5):
        model = TSNE(n_components=2, perplexity=s["perplexity"], max_iter=s["max_iter"], init=y0.astype(np.float32), angle=angle,
                     method="barnes_hut", random_state=42)
        y = model.fit_transform(x.astype(np.float64))
        runs[f"sklearn_angle_{angle:g}"] = {"kl": float(model.kl_divergence_),
                                            "trustworthiness": float(R.trustworthiness(x, y, s["trust_neighbors"]))}
    rng = np.random.default_rng(s["seed"])
    rand = rng.normal(size=(s["m"], 2)) * layouts["restatement_float64"].std()
    random_layout = {"kl": float(R.gradient(rand, *p)[2]), "trustworthiness": float(R.trustworthiness(x, rand, s["trust_neighbors"]))}
    out = {"setting": s, "runs": runs, "random_layout": random_layout}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_blobs300.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
