"""Writes tests/golden/reduce_item_parent.npz: the hub rows, and the SHA-1 of the whole output, of the two-launch gather on
the seeded float tables of tests/test_reduce_item_early_cnt.py.  Run it on a GPU with the library built from the commit
BEFORE the divisor of rgcn_reduce_item moved in front of the row loads: the test holds every later build to these bytes.

    python tests/golden/make_reduce_item_golden.py [OUT.npz]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import test_reduce_item_early_cnt as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    dev = torch.device("cuda:0")
    arrays = {}
    for name in ("in", "out"):
        s = T.side(name)
        for d in (64, 128):
            got = s.gather(torch.from_numpy(T.table("floats", d)).to(dev)).cpu().numpy()
            arrays[f"{name}_d{d}_hub_rows"] = got.reshape(T.N_NODES * T.R, d)[s.hub_rows].copy()
            arrays[f"{name}_d{d}_sha1"] = T.digest(got)
    np.savez(out, **arrays)
    print("wrote", out, {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
