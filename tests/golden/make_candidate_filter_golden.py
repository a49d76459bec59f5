"""Writes tests/golden/candidate_filter_parent.npz: per case of tests/test_candidate_filter_parent_bits.py and per output
buffer, the SHA-1 of the buffer and its first four rows.  Run it on a GPU with the library and ops.py of the commit BEFORE
the ranking, top-k and softmax passes moved onto the one candidate-filter frame (csrc/rgcn_candidate_filter.h, the chunk
generator of ops.py): the test holds every later build to these bytes.  Only buffers that two runs reproduce are recorded.
Never re-record it to make a later build pass.

    python tests/golden/make_candidate_filter_golden.py [OUT.npz]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import test_candidate_filter_parent_bits as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    dev = torch.device("cuda:0")
    arrays = {}
    for name in sorted(T.CASES):
        first = T.outputs(name, dev)
        again = T.outputs(name, dev)
        for key, a in first.items():
            assert a.tobytes() == again[key].tobytes(), f"{name}/{key}: two runs differ, nothing to record"
            arrays[f"{name}/{key}_sha1"] = T.digest(a)
            arrays[f"{name}/{key}_rows"] = T.head_rows(a)
    np.savez(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")
    for k, v in arrays.items():
        print(" ", k, v.dtype, v.shape)


if __name__ == "__main__":
    main()
