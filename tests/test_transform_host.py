"""CPU tier of the dense transforms' host side (``csrc/rgcn_transform_host.h``, the entry points of
``rgcn_transform.hip`` / ``rgcn_transform_split.hip`` / ``rgcn_transform_f16.hip``).  No GPU: every call below is
rejected - or, with ``N == 0``, answered - before the library touches the device.

``ROWS`` is the return code of every transform entry point for each way a call can be wrong, several ways at once
included (which pins the ORDER of the checks); ``tests/golden/transform_host_sizes.json`` holds the workspace and
packed-weight sizes over a grid.  Both were recorded with the library as it stood BEFORE the host side was folded into
one header and one call descriptor, and must not move: Python sizes its arenas from these queries.
(The ``N == 0`` path of the two parameter-gradient ``begin`` calls clears the gradients on the device, so it is left to
the GPU tier; here ``N == 0`` is only followed as far as the workspace check.)

``tests/transform_host_check.cpp`` holds ``rgcn_tn_plan`` to a verbatim copy of the two planners it replaced, over the
same grid, as a stand-alone program under AddressSanitizer / UndefinedBehaviorSanitizer."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from primekg_rgcn_linkprediction_amd import _lib

OK, A, U, W = _lib.RGCN_OK, _lib.RGCN_ERR_ARG, _lib.RGCN_ERR_UNSUPPORTED, _lib.RGCN_ERR_WORKSPACE
P = 256                      # "some device pointer": never dereferenced by a call that is rejected on the host
NAN = float("nan")
BIG_N = 1 << 30              # > INT32_MAX / 2
BIG_D = 1 << 23              # (R + 1) * BIG_D > 1 << 24 for every R >= 1; a multiple of 64
PACK_JOBS = 4                # RGCN_PACK_JOBS (csrc/rgcn_prep.h)

SIZES = os.path.join(GOLDEN, "transform_host_sizes.json")
GRID_N = [0, 1, 31, 32, 33, 127, 128, 129, 4096, 30926, 262144, 4_200_000]
GRID_R = [1, 3, 33]
GRID_D = [4, 32, 64, 96, 128, 256]

# entry point -> its parameters in order, each with the value of a call that is RIGHT ("ws_bytes": None = exactly what
# the entry point's own query asks for; "short": one byte less)
GOOD = {
    "rgcn_transform_fwd": dict(agg=P, x=P, weight=P, root=P, bias=None, relu=0, tile_mask=None, N=10, R=3, d_in=64,
                               d_out=64, out=P, stream=None),
    "rgcn_transform_bwd_input": dict(gagg=P, g=P, weight=P, root=P, relu_mask=None, tile_mask=None, N=10, R=3, d_in=64,
                                     d_out=64, grad_x=P, stream=None),
    "rgcn_transform_bwd_params": dict(agg=P, x=P, g=P, tile_mask=None, N=10, R=3, d_in=64, d_out=64, grad_weight=P,
                                      grad_root=P, grad_bias=P, ws=P, ws_bytes=None, stream=None),
    "rgcn_transform_bwd_params_begin": dict(agg=P, x=P, g=P, tile_mask=None, N=10, R=3, d_in=64, d_out=64, grad_weight=P,
                                            grad_root=P, grad_bias=P, ws=P, ws_bytes=None, stream=None, job="job"),
    "rgcn_transform_fwd_f16": dict(agg=P, x=P, weight=P, root=P, bias=None, relu=0, tile_mask=None, N=10, R=3, d_in=64,
                                   d_out=64, out=P, ws=P, ws_bytes=None, stream=None),
    "rgcn_transform_fwd_split": dict(agg=P, x=P, weight=P, root=P, packed=None, bias=None, relu=0, tile_mask=None, N=10,
                                     R=3, d_in=64, d_out=64, agg_amax=None, agg_amax_mul=1.0, x_amax=None, half=0,
                                     out=P, out_amax=None, ws=P, ws_bytes=None, stream=None, hub_graph=None,
                                     hub_transposed=0, hub_partial=None),
    "rgcn_transform_bwd_input_split": dict(gagg=P, g=P, weight=P, root=P, packed=None, relu_mask=None, tile_mask=None,
                                           N=10, R=3, d_in=64, d_out=64, gagg_amax=None, gagg_amax_mul=1.0, g_amax=None,
                                           half=0, grad_x=P, grad_x_amax=None, ws=P, ws_bytes=None, stream=None,
                                           hub_graph=None, hub_transposed=0, hub_partial=None, out_scale=1.0),
    "rgcn_transform_bwd_input_chain_split": dict(gagg=P, g=P, weight=P, root=P, packed=P, relu_mask=None, tile_mask=None,
                                                 N=10, R=3, d_in=128, d_out=64, gagg_amax=P, gagg_amax_mul=1.0,
                                                 g_amax=P, grad_x=P, grad_x_amax=None, ws=P, ws_bytes=None, stream=None,
                                                 hub_graph=None, hub_transposed=0, hub_partial=None, out_scale=1.0,
                                                 packed1=P, has_root1=1, R1=3, d_in1=64, t_out=P),
    "rgcn_transform_first_split": dict(g=P, packed=P, has_root=1, N=10, R=3, d_in=64, d_out=64, g_amax=None, half=0,
                                       t_out=P, ws=P, ws_bytes=None, stream=None),
    "rgcn_transform_bwd_params_split_begin": dict(agg=P, x=P, g=P, tile_mask=None, N=10, R=3, d_in=64, d_out=64,
                                                  agg_amax=None, agg_amax_mul=1.0, x_amax=None, g_amax=None, half=0,
                                                  grad_weight=P, grad_root=P, grad_bias=P, ws=P, ws_bytes=None,
                                                  stream=None, job="job"),
    "rgcn_weights_split_pack": dict(weight=P, root=P, R=3, d_in=64, d_out=64, ws=P, ws_bytes=None, stream=None),
}


def _ws_bytes(lib, name, a):
    """what the entry point's own workspace query asks for the call ``a``"""
    if name in ("rgcn_transform_bwd_params", "rgcn_transform_bwd_params_begin"):
        return lib.rgcn_transform_bwd_params_workspace_bytes(a["N"], a["R"], a["d_in"], a["d_out"])
    if name == "rgcn_transform_bwd_params_split_begin":
        return lib.rgcn_transform_bwd_params_split_workspace_bytes(a["N"], a["R"], a["d_in"], a["d_out"])
    if name == "rgcn_transform_fwd_f16":
        return lib.rgcn_transform_fwd_f16_workspace_bytes(a["R"], a["d_in"], a["d_out"])
    if name == "rgcn_transform_first_split":
        return 2048                                              # two rows of partial maxima (ops.transform_first)
    if name == "rgcn_weights_split_pack":
        return lib.rgcn_weights_split_bytes(a["R"], a["d_in"], a["d_out"])
    return lib.rgcn_transform_split_workspace_bytes(a["R"], a["d_in"], a["d_out"])


def _call(lib, name, wrong):
    a = dict(GOOD[name])
    assert wrong and set(wrong) <= set(a), (name, wrong)          # a row changes something, and only what exists
    a.update(wrong)
    if "ws_bytes" in a and a["ws_bytes"] in (None, "short"):
        a["ws_bytes"] = max(0, _ws_bytes(lib, name, a) - (a["ws_bytes"] == "short"))
    job = _lib.SlabJob(slab=P, bias_part=P, splits=7, K1=7, Kc=7, N=7, grad_weight=P, grad_root=P, grad_bias=P)
    if a.get("job") == "job":
        a["job"] = ctypes.byref(job)
    rc = getattr(lib, name)(*a.values())
    if "job" in a and a["job"] is not None:                       # a refused call leaves an EMPTY job behind, not the old one
        assert (job.slab, job.bias_part, job.splits, job.K1, job.Kc, job.N, job.grad_weight) == (None, None, 0, 0, 0, 0, None)
    return rc


NT = ("rgcn_transform_fwd", "rgcn_transform_bwd_input", "rgcn_transform_fwd_f16", "rgcn_transform_fwd_split",
      "rgcn_transform_bwd_input_split")
OUT = {"rgcn_transform_fwd": "out", "rgcn_transform_bwd_input": "grad_x", "rgcn_transform_fwd_f16": "out",
       "rgcn_transform_fwd_split": "out", "rgcn_transform_bwd_input_split": "grad_x",
       "rgcn_transform_bwd_input_chain_split": "grad_x", "rgcn_transform_first_split": "t_out",
       "rgcn_transform_bwd_params": "grad_weight", "rgcn_transform_bwd_params_begin": "grad_weight",
       "rgcn_transform_bwd_params_split_begin": "grad_weight"}
FIRST_OPERAND = {"rgcn_transform_fwd": "agg", "rgcn_transform_bwd_input": "gagg", "rgcn_transform_fwd_f16": "x",
                 "rgcn_transform_fwd_split": "weight", "rgcn_transform_bwd_input_split": "g",
                 "rgcn_transform_bwd_input_chain_split": "gagg", "rgcn_transform_first_split": "g",
                 "rgcn_transform_bwd_params": "g", "rgcn_transform_bwd_params_begin": "agg",
                 "rgcn_transform_bwd_params_split_begin": "x"}

# (entry point, what is wrong with the call, the code the library returned before the refactor)
ROWS = []
for _name in OUT:                                                 # what every layer call shares
    ROWS += [
        (_name, dict(d_in=62), A),                                # a dimension that is no multiple of 4
        (_name, dict(d_out=62), A),
        (_name, dict(R=0), A),
        (_name, dict(N=-1), A),
        (_name, {OUT[_name]: None}, A),                           # no output
        (_name, {FIRST_OPERAND[_name]: None}, A),                 # a missing operand with N > 0
        (_name, {OUT[_name]: None, "N": 0}, A),
        (_name, dict(N=BIG_N), U),
        (_name, dict(d_in=62, N=BIG_N, **{OUT[_name]: None}), A),            # ... the dimensions come first
        (_name, {FIRST_OPERAND[_name]: None, "N": BIG_N}, A),                # ... operands before the range
    ]
for _name in NT + ("rgcn_transform_first_split",):                # N == 0: nothing to do, whatever else is missing
    ROWS += [(_name, {"N": 0, FIRST_OPERAND[_name]: None}, OK)]
    if "ws" in GOOD[_name]:
        ROWS += [(_name, dict(N=0, ws=None, ws_bytes=0), OK)]
ROWS += [
    # ---- fp32
    ("rgcn_transform_fwd", dict(d_in=BIG_D), U),                                  # (R + 1) * d_in over 1 << 24
    ("rgcn_transform_fwd", dict(d_out=(1 << 24) + 4), U),
    ("rgcn_transform_fwd", dict(d_out=1 << 24, out=None), A),
    ("rgcn_transform_bwd_input", dict(d_out=BIG_D), U),                           # here d_out is the reduction width
    ("rgcn_transform_bwd_input", dict(d_in=(1 << 24) + 4), U),
    ("rgcn_transform_bwd_input", dict(d_in=BIG_D, d_out=4, R=1, N=0), OK),
    ("rgcn_transform_bwd_params", dict(d_in=BIG_D), U),
    ("rgcn_transform_bwd_params", dict(ws=None), W),
    ("rgcn_transform_bwd_params", dict(ws_bytes="short"), W),
    ("rgcn_transform_bwd_params", dict(N=0, agg=None, x=None, g=None, ws=None), W),    # N == 0 skips the operands only
    ("rgcn_transform_bwd_params", dict(d_in=BIG_D, ws=None), U),
    ("rgcn_transform_bwd_params_begin", dict(job=None, d_in=62, grad_weight=None), A),
    ("rgcn_transform_bwd_params_begin", dict(d_in=BIG_D), U),
    ("rgcn_transform_bwd_params_begin", dict(d_out=(1 << 24) + 4), U),
    ("rgcn_transform_bwd_params_begin", dict(ws=None), W),
    ("rgcn_transform_bwd_params_begin", dict(ws_bytes="short"), W),
    ("rgcn_transform_bwd_params_begin", dict(ws_bytes="short", N=4_200_000, d_in=128, d_out=128), W),
    ("rgcn_transform_bwd_params_begin", dict(ws_bytes="short", grad_root=None, grad_bias=None), W),   # sized for the root anyway
    ("rgcn_transform_bwd_params_begin", dict(N=0, agg=None, x=None, g=None, ws=None), W),
    ("rgcn_transform_bwd_params_begin", dict(N=BIG_N, ws=None), U),
    ("rgcn_transform_bwd_params_begin", dict(g=None, ws=None, d_in=BIG_D), A),
    ("rgcn_transform_bwd_params_begin", dict(d_in=36, ws=None), W),                # no K rule of its own: any multiple of 4
    # ---- fp16 operands
    ("rgcn_transform_fwd_f16", dict(d_in=48), U),                                 # a k-tile would straddle two relations
    ("rgcn_transform_fwd_f16", dict(d_in=BIG_D), U),
    ("rgcn_transform_fwd_f16", dict(ws=None), W),
    ("rgcn_transform_fwd_f16", dict(ws_bytes="short"), W),
    ("rgcn_transform_fwd_f16", dict(d_in=48, ws=None), U),
    ("rgcn_transform_fwd_f16", dict(d_in=48, agg=None), A),
    ("rgcn_transform_fwd_f16", dict(N=BIG_N, ws=None), U),
    # ---- split precision, forward
    ("rgcn_transform_fwd_split", dict(d_in=48), U),
    ("rgcn_transform_fwd_split", dict(d_in=BIG_D), U),
    ("rgcn_transform_fwd_split", dict(d_out=(1 << 24) + 4), U),
    ("rgcn_transform_fwd_split", dict(ws=None), W),
    ("rgcn_transform_fwd_split", dict(ws_bytes="short"), W),
    ("rgcn_transform_fwd_split", dict(ws_bytes="short", packed=P), W),            # the same size with the weights brought along
    ("rgcn_transform_fwd_split", dict(d_in=48, ws=None), U),
    ("rgcn_transform_fwd_split", dict(d_in=48, x=None), A),
    ("rgcn_transform_fwd_split", dict(N=BIG_N, ws=None), U),
    ("rgcn_transform_fwd_split", dict(d_in=62, ws=None, N=BIG_N), A),
    # ---- split precision, input gradient
    ("rgcn_transform_bwd_input_split", dict(out_scale=0.0), A),
    ("rgcn_transform_bwd_input_split", dict(out_scale=NAN), A),
    ("rgcn_transform_bwd_input_split", dict(out_scale=-1.0), A),
    ("rgcn_transform_bwd_input_split", dict(out_scale=0.0, N=0), A),               # ... before N == 0
    ("rgcn_transform_bwd_input_split", dict(out_scale=NAN, d_out=48, ws=None), A),
    ("rgcn_transform_bwd_input_split", dict(d_out=48), U),                         # d_out is the k width here
    ("rgcn_transform_bwd_input_split", dict(d_in=36, ws=None), W),                 # ... and d_in is free
    ("rgcn_transform_bwd_input_split", dict(d_out=BIG_D), U),
    ("rgcn_transform_bwd_input_split", dict(d_in=(1 << 24) + 4), U),
    ("rgcn_transform_bwd_input_split", dict(ws=None), W),
    ("rgcn_transform_bwd_input_split", dict(ws_bytes="short"), W),
    ("rgcn_transform_bwd_input_split", dict(d_out=48, ws=None), U),
    ("rgcn_transform_bwd_input_split", dict(d_out=48, gagg=None), A),
    # ---- split precision, input gradient with the chained product
    ("rgcn_transform_bwd_input_chain_split", dict(d_in=64), U),                    # built for d_in == 128
    ("rgcn_transform_bwd_input_chain_split", dict(d_in=256), U),
    ("rgcn_transform_bwd_input_chain_split", dict(packed1=None), A),
    ("rgcn_transform_bwd_input_chain_split", dict(packed=None), A),
    ("rgcn_transform_bwd_input_chain_split", dict(t_out=None), A),
    ("rgcn_transform_bwd_input_chain_split", dict(packed1=None, d_in=64), A),
    ("rgcn_transform_bwd_input_chain_split", dict(out_scale=0.0), A),
    ("rgcn_transform_bwd_input_chain_split", dict(out_scale=NAN, d_in=64), A),
    ("rgcn_transform_bwd_input_chain_split", dict(d_in=64, N=0), U),               # supported or not comes before N == 0
    ("rgcn_transform_bwd_input_chain_split", dict(N=0, gagg=None, g=None, weight=None, gagg_amax=None, ws=None), OK),
    ("rgcn_transform_bwd_input_chain_split", dict(d_out=48), U),
    ("rgcn_transform_bwd_input_chain_split", dict(R1=0), U),
    ("rgcn_transform_bwd_input_chain_split", dict(d_in1=62), U),
    ("rgcn_transform_bwd_input_chain_split", dict(gagg_amax=None), A),             # the chain scans nothing itself
    ("rgcn_transform_bwd_input_chain_split", dict(g_amax=None, N=BIG_N), A),
    ("rgcn_transform_bwd_input_chain_split", dict(d_out=BIG_D), U),
    ("rgcn_transform_bwd_input_chain_split", dict(d_in1=BIG_D), U),
    ("rgcn_transform_bwd_input_chain_split", dict(ws=None), W),
    ("rgcn_transform_bwd_input_chain_split", dict(ws_bytes="short"), W),
    ("rgcn_transform_bwd_input_chain_split", dict(d_in1=BIG_D, ws=None), U),
    # ---- split precision, transform first
    ("rgcn_transform_first_split", dict(packed=None), A),
    ("rgcn_transform_first_split", dict(d_out=48), U),
    ("rgcn_transform_first_split", dict(d_in=BIG_D), U),                           # the output columns (R + 1) * d_in
    ("rgcn_transform_first_split", dict(d_out=(1 << 24) + 32), U),
    ("rgcn_transform_first_split", dict(ws=None), W),
    ("rgcn_transform_first_split", dict(ws_bytes=2047), W),
    ("rgcn_transform_first_split", dict(d_out=48, ws=None), U),
    ("rgcn_transform_first_split", dict(packed=None, N=0), A),
    # ---- split precision, parameter gradients
    ("rgcn_transform_bwd_params_split_begin", dict(job=None, d_in=62, grad_weight=None), A),
    ("rgcn_transform_bwd_params_split_begin", dict(d_in=32), U),                   # a 64-column kc tile lies in one relation
    ("rgcn_transform_bwd_params_split_begin", dict(d_in=96), U),
    ("rgcn_transform_bwd_params_split_begin", dict(d_in=BIG_D), U),
    ("rgcn_transform_bwd_params_split_begin", dict(d_out=(1 << 24) + 4), U),
    ("rgcn_transform_bwd_params_split_begin", dict(ws=None), W),
    ("rgcn_transform_bwd_params_split_begin", dict(ws_bytes="short"), W),
    ("rgcn_transform_bwd_params_split_begin", dict(ws_bytes="short", N=4_200_000, d_in=128, d_out=128), W),
    ("rgcn_transform_bwd_params_split_begin", dict(ws_bytes="short", grad_root=None, grad_bias=None), W),
    ("rgcn_transform_bwd_params_split_begin", dict(N=0, agg=None, x=None, g=None, ws=None), W),
    ("rgcn_transform_bwd_params_split_begin", dict(d_in=32, ws=None), U),
    ("rgcn_transform_bwd_params_split_begin", dict(d_in=32, x=None), A),
    ("rgcn_transform_bwd_params_split_begin", dict(d_in=32, N=0, x=None), U),
    # ---- the split weights of one layer
    ("rgcn_weights_split_pack", dict(R=0), A),
    ("rgcn_weights_split_pack", dict(d_in=0), A),
    ("rgcn_weights_split_pack", dict(d_out=-4), A),
    ("rgcn_weights_split_pack", dict(weight=None), A),
    ("rgcn_weights_split_pack", dict(d_in=BIG_D), U),
    ("rgcn_weights_split_pack", dict(d_out=BIG_D), U),
    ("rgcn_weights_split_pack", dict(ws=None), W),
    ("rgcn_weights_split_pack", dict(ws_bytes="short"), W),
    ("rgcn_weights_split_pack", dict(weight=None, d_in=BIG_D, ws=None), A),
    ("rgcn_weights_split_pack", dict(d_out=BIG_D, ws=None), U),
]


def test_rows_cover_every_entry_point_and_none_reaches_the_device():
    assert {name for name, _, _ in ROWS} == set(GOOD)
    assert all(code in (OK, A, U, W) for _, _, code in ROWS)       # never RGCN_ERR_HIP: that would have been a device call
    assert all(code != OK or wrong.get("N") == 0 for _, wrong, code in ROWS)


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_transform_entry_point_returns_the_recorded_code(row):
    name, wrong, code = ROWS[row]
    assert _call(_lib.load(), name, wrong) == code, (name, wrong)


# ------------------------------------------------------------------ the packs of several layers, the pending reduction
def _layers(lib, count, **wrong):
    """host arrays of a ``count``-layer pack call, every layer right except what ``wrong`` says about the LAST one"""
    n = max(count, 1)
    last = dict(weight=P, root=P, R=3, d_in=64, d_out=64, packed=P, short=0)
    last.update(wrong)
    rows = [dict(weight=P, root=P, R=3, d_in=64, d_out=64, packed=P, short=0)] * (n - 1) + [last]
    ptrs = lambda key: (ctypes.c_void_p * n)(*[r[key] for r in rows])
    ints = lambda key: (ctypes.c_int64 * n)(*[r[key] for r in rows])
    need = [lib.rgcn_weights_split_bytes(r["R"], r["d_in"], r["d_out"]) - r["short"] for r in rows]
    return dict(weights=ptrs("weight"), roots=ptrs("root"), R=ints("R"), d_in=ints("d_in"), d_out=ints("d_out"),
                packed=ptrs("packed"), packed_bytes=(ctypes.c_size_t * n)(*[max(0, b) for b in need]))


# (layers, what is wrong with the last layer, what else is wrong with the call, code)
PACK_ROWS = [
    (0, {}, {}, A),
    (PACK_JOBS + 1, {}, {}, A),
    (1, dict(R=0), {}, A),
    (2, dict(d_in=0), {}, A),
    (2, dict(d_out=62), {}, A),                                   # (the single-layer call does not ask this)
    (2, dict(weight=None), {}, A),
    (2, dict(d_in=BIG_D), {}, U),
    (PACK_JOBS, dict(d_out=BIG_D), {}, U),
    (2, dict(packed=None), {}, W),
    (2, dict(short=1), {}, W),
    (1, dict(short=1), {}, W),
    (2, dict(d_out=62, d_in=BIG_D, packed=None), {}, A),
    (2, dict(d_in=BIG_D, packed=None), {}, U),
    (2, dict(weight=None, short=1), {}, A),
    (2, dict(short=1), dict(zero_count=-1), A),                   # the call's own arguments before any layer
    (2, dict(short=1), dict(zero_count=1, zero_buffers=None), A),
    (2, dict(short=1), dict(zero_count=1025, zero_buffers=P), A),
    (2, dict(short=1), dict(zero_count=1024, zero_buffers=P), W),
    (2, dict(short=1), dict(R=None), A),
    (PACK_JOBS + 1, dict(R=0), dict(zero_count=-1), A),
]


@pytest.mark.parametrize("row", range(len(PACK_ROWS)))
def test_pack_of_several_layers_returns_the_recorded_code(row):
    lib = _lib.load()
    count, wrong, call, code = PACK_ROWS[row]
    a = _layers(lib, count, **wrong)
    a.update({k: v for k, v in call.items() if k in a})
    zc, zb = call.get("zero_count", 0), call.get("zero_buffers")
    multi = lib.rgcn_weights_split_pack_multi(count, a["weights"], a["roots"], a["R"], a["d_in"], a["d_out"], None, None,
                                              a["packed"], a["packed_bytes"], zb, zc, None)
    fill = lib.rgcn_absmax_pack(P, 100, P, zb, zc, count, a["weights"], a["roots"], a["R"], a["d_in"], a["d_out"],
                                a["packed"], a["packed_bytes"], None)
    assert (multi, fill) == (code, code)


def test_absmax_pack_checks_its_table_before_the_layers():
    lib = _lib.load()
    a = _layers(lib, 2, short=1)
    call = lambda x, numel, x_amax: lib.rgcn_absmax_pack(x, numel, x_amax, None, 0, 2, a["weights"], a["roots"], a["R"],
                                                         a["d_in"], a["d_out"], a["packed"], a["packed_bytes"], None)
    assert (call(P, -1, P), call(P, 100, None), call(None, 100, P), call(None, 0, P)) == (A, A, A, W)


def test_pending_reduction_checks_its_job():
    lib = _lib.load()
    good = dict(slab=P, bias_part=P, splits=2, K1=192, Kc=256, N=64, grad_weight=P, grad_root=P, grad_bias=P)
    assert lib.rgcn_slab_reduce(None, None) == A
    assert lib.rgcn_slab_reduce(ctypes.byref(_lib.SlabJob()), None) == OK                      # nothing pending
    assert lib.rgcn_slab_reduce(ctypes.byref(_lib.SlabJob(**dict(good, slab=None, splits=0))), None) == OK
    for wrong in (dict(grad_weight=None), dict(splits=0), dict(Kc=0), dict(N=0), dict(N=62), dict(N=-4)):
        assert lib.rgcn_slab_reduce(ctypes.byref(_lib.SlabJob(**dict(good, **wrong))), None) == A, wrong


def test_chain_supported_is_the_recorded_predicate():
    lib = _lib.load()
    q = lib.rgcn_transform_bwd_input_chain_supported
    assert [q(3, 128, 64, 3, 64), q(1, 128, 32, 1, 4), q(3, 128, 128, 33, 256)] == [1, 1, 1]
    assert [q(0, 128, 64, 3, 64), q(3, 128, 64, 0, 64), q(3, 64, 64, 3, 64), q(3, 256, 64, 3, 64), q(3, 128, 48, 3, 64),
            q(3, 128, 0, 3, 64), q(3, 128, 64, 3, 62), q(3, 128, 64, 3, 0)] == [0] * 8


# ------------------------------------------------------------------ sizes
def _sizes(lib):
    per_layer = [(r, di, do) for r in GRID_R for di in GRID_D for do in GRID_D]
    per_graph = [(n, r, di, do) for n in GRID_N for (r, di, do) in per_layer]
    return {
        "rgcn_transform_bwd_params_workspace_bytes": [lib.rgcn_transform_bwd_params_workspace_bytes(*c) for c in per_graph],
        "rgcn_transform_bwd_params_split_workspace_bytes":
            [lib.rgcn_transform_bwd_params_split_workspace_bytes(*c) for c in per_graph],
        "rgcn_transform_split_workspace_bytes": [lib.rgcn_transform_split_workspace_bytes(*c) for c in per_layer],
        "rgcn_transform_fwd_f16_workspace_bytes": [lib.rgcn_transform_fwd_f16_workspace_bytes(*c) for c in per_layer],
        "rgcn_weights_split_bytes": [lib.rgcn_weights_split_bytes(*c) for c in per_layer],
    }


def test_workspace_and_packed_sizes_have_not_moved_by_a_byte():
    """N x R x d_in x d_out over both sides of the two-workgroups-per-CU threshold and of ``splits == 1``"""
    recorded = json.load(open(SIZES))
    assert (recorded["N"], recorded["R"], recorded["d"]) == (GRID_N, GRID_R, GRID_D)
    now = _sizes(_lib.load())
    assert sorted(now) == sorted(recorded["bytes"])
    for name, values in now.items():
        assert len(values) == len(recorded["bytes"][name]) and len(values) in (108, 1296)
        moved = [i for i, (a, b) in enumerate(zip(values, recorded["bytes"][name])) if a != b]
        assert not moved, f"{name}: {len(moved)} of {len(values)} sizes moved, first at grid index {moved[0]}"
    # the grid sees both plans' branches: one split and many, 256 and 512 target workgroups
    fp32 = recorded["bytes"]["rgcn_transform_bwd_params_workspace_bytes"]
    at = lambda n, r, di, do: fp32[((GRID_N.index(n) * 3 + GRID_R.index(r)) * 6 + GRID_D.index(di)) * 6 + GRID_D.index(do)]
    assert at(1, 3, 128, 128) == (1 * 512 * 128 + 128) * 4                         # one split
    assert at(30926, 3, 128, 128) == 32 * (512 * 128 + 128) * 4                    # 256 workgroups over 8 tiles
    assert at(262144, 3, 128, 128) == 64 * (512 * 128 + 128) * 4                   # 512: >= 2,048 rows each
    assert at(4_200_000, 3, 128, 128) == 64 * (512 * 128 + 128) * 4
    assert lib_zero_sizes(_lib.load()) == [0] * 8


def lib_zero_sizes(lib):
    """the queries answer 0 for dimensions no call accepts"""
    return [lib.rgcn_transform_bwd_params_workspace_bytes(-1, 3, 64, 64), lib.rgcn_transform_bwd_params_workspace_bytes(10, 0, 64, 64),
            lib.rgcn_transform_bwd_params_split_workspace_bytes(-1, 3, 64, 64),
            lib.rgcn_transform_bwd_params_split_workspace_bytes(10, 3, 0, 64), lib.rgcn_transform_split_workspace_bytes(0, 64, 64),
            lib.rgcn_transform_fwd_f16_workspace_bytes(3, 64, 0), lib.rgcn_weights_split_bytes(3, -64, 64),
            lib.rgcn_weights_split_bytes(0, 64, 64)]


# ------------------------------------------------------------------ the shared header, as host code
def _csrc(name):
    return os.path.join(ROOT, "primekg_rgcn_linkprediction_amd", "csrc", name)


def test_tn_plan_is_both_former_planners_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "transform_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", ROOT,
                    os.path.join(ROOT, "tests", "transform_host_check.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    last = done.stdout.strip().splitlines()[-1] if done.stdout.strip() else ""
    assert done.returncode == 0 and last == "transform_host_check ok 1296 shapes", done.stdout[-2000:] + done.stderr[-2000:]


def test_transform_host_header_has_no_device_code_and_the_three_files_use_it():
    header = open(_csrc("rgcn_transform_host.h")).read()
    assert "hip_runtime" not in header and "__global__" not in header and "__device__" not in header
    for name in ("rgcn_transform.hip", "rgcn_transform_split.hip", "rgcn_transform_f16.hip"):
        text = open(_csrc(name)).read()
        assert '#include "rgcn_transform_host.h"' in text, name
        for gone in ("bad_dims(int64_t", "struct SplitPlan", "struct TnPlan", "plan_splits(", " tn_plan(", "(1 << 24)"):
            assert gone not in text, (name, gone)                  # one copy each: the header's


if __name__ == "__main__":                                        # records the sizes of the library that is built NOW
    _lib_ = _lib.load()
    json.dump({"N": GRID_N, "R": GRID_R, "d": GRID_D, "bytes": _sizes(_lib_)}, open(SIZES, "w"), separators=(",", ":"))
    print("wrote", SIZES)
