"""The split weight images and the maxima of a pass's first launch, byte for byte.

Every entry point that reaches the pack body (``rgcn_absmax_pack``, ``rgcn_weights_split_pack``,
``rgcn_weights_split_pack_multi`` with and without given maxima) writes into a buffer pre-filled with 0xFF; the whole
buffer - images, the inverse scale, the padding between them and whatever the launch must leave alone - is compared
with a numpy restatement of the definitions: ``scale_exponent`` / ``pow2f`` of ``csrc/rgcn_split.h``, fp16
round-to-nearest-even, and the five index formulas of ``csrc/rgcn_prep.h`` / ``rgcn_split.h``.  Nothing here is taken
from the library under test."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import need_gpu
from primekg_rgcn_linkprediction_amd import _lib, ops

pytestmark = pytest.mark.gpu

AMAX_FLOATS, HEADS, HEAD_STRIDE = 2048, 256, 8
MAX_SLOTS = 256                      # partial maxima behind the inverse scale (2 * MAX_SLOTS floats, never written by a pack)


# ------------------------------------------------------------------------------------------------ the definitions
def scale_exponent(amax):
    bits = int(np.float32(amax).view(np.uint32))
    e = (bits >> 23) & 0xFF
    if e == 0 or e == 255:
        return 0
    return max(-100, min(100, 141 - e))


def pow2f(s):
    return np.uint32((127 + s) << 23).view(np.float32)


def packed_bytes(r, d_in, d_out):
    img = -(-((r + 1) * d_in * d_out * 2) // 256) * 256
    return 10 * img + 256 + 2 * MAX_SLOTS * 4


def fragment_order(image):
    """image[n][k] (n % 32 == 0, k % 16 == 0) -> element ((s * NT + nt) * 64 + lane) * 8 + j =
    image[32 nt + (lane & 31)][16 s + 8 (lane >> 5) + j]"""
    n, k = image.shape
    e = np.arange(n * k)
    j, lane, blk = e & 7, (e >> 3) & 63, e >> 9
    nt = n // 32
    return image[32 * (blk % nt) + (lane & 31), 16 * (blk // nt) + 8 * (lane >> 5) + j]


def expected_buffer(w, root):
    """the packed buffer of one layer after a pack into 0xFF bytes (w: [R, d_in, d_out] float32, root: [d_in, d_out] | None)"""
    r, d_in, d_out = w.shape
    full = w if root is None else np.concatenate([w, root[None]], axis=0)          # [blocks, d_in, d_out]
    blocks = full.shape[0]
    amax = np.float32(np.abs(full).max()) if full.size else np.float32(0)
    eb = scale_exponent(amax)
    with np.errstate(over="ignore", under="ignore"):
        v = (full * pow2f(eb)).astype(np.float32)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    images = []
    for part in (hi, lo):                                                          # forward [o][r d_in + i]
        images.append(part.transpose(2, 0, 1).reshape(d_out, blocks * d_in))
    for part in (hi, lo):                                                          # backward [i][r d_out + o]
        images.append(part.transpose(1, 0, 2).reshape(d_in, blocks * d_out))
    if d_in % 32 == 0 and d_out % 32 == 0:
        frag = [fragment_order(images[0]), fragment_order(images[1]), fragment_order(images[2]), fragment_order(images[3])]
    else:
        frag = [None] * 4                                                          # the element-wise body writes none
    images = [im.reshape(-1) for im in images] + frag + [hi.reshape(-1), lo.reshape(-1)]   # natural [(r, i)][o]
    buf = np.full(packed_bytes(r, d_in, d_out), 0xFF, dtype=np.uint8)
    img = -(-((r + 1) * d_in * d_out * 2) // 256) * 256
    for k, im in enumerate(images):
        if im is not None:
            raw = np.ascontiguousarray(im).view(np.uint8)
            buf[k * img: k * img + raw.size] = raw
    buf[10 * img: 10 * img + 4] = np.array([pow2f(-eb)], dtype=np.float32).view(np.uint8)
    return buf


# ------------------------------------------------------------------------------------------------ the layers
def _layer(seed, r, d_in, d_out, root=True, kind="random"):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((r, d_in, d_out)) * 0.1).astype(np.float32)
    rt = (rng.standard_normal((d_in, d_out)) * 0.1).astype(np.float32) if root else None
    # a few values far below the maximum: the lo half goes subnormal, the hi half to zero
    w.reshape(-1)[:: 7] *= np.float32(2.0 ** -18)
    w.reshape(-1)[3:: 11] *= np.float32(2.0 ** -30)
    if kind == "max_last":                       # the maximum is the very last element of [W ; root]
        (rt if root else w).reshape(-1)[-1] = -3.75
    elif kind == "max_in_root":
        rt[d_in // 2, d_out // 3] = 5.5
    elif kind == "zero":
        w[:] = 0
        if root:
            rt[:] = 0
    return w, rt


C2_1, C2_2 = (3, 64, 128), (3, 128, 128)
CALLS = {
    "one_tile": [_layer(1, 1, 32, 32)],
    "c2_pair": [_layer(2, *C2_1), _layer(3, *C2_2)],
    "four_layers": [_layer(4, *C2_1), _layer(5, *C2_2), _layer(6, 2, 32, 96, root=False), _layer(7, 2, 36, 20)],
    "no_root": [_layer(8, 2, 32, 96, root=False)],
    "fallback_36_20": [_layer(9, 2, 36, 20)],
    "fallback_4_4": [_layer(10, 1, 4, 4)],
    "max_last": [_layer(11, 3, 64, 128, kind="max_last"), _layer(12, 2, 32, 96, root=False, kind="max_last")],
    "max_in_root": [_layer(13, 3, 128, 128, kind="max_in_root")],
    "all_zero": [_layer(14, 2, 64, 32, kind="zero"), _layer(15, 1, 4, 4, kind="zero")],
}
ENTRIES = ["absmax_pack", "multi_scan", "multi_given", "single"]

_EXPECTED = {}


def _expected(name):
    if name not in _EXPECTED:
        _EXPECTED[name] = [expected_buffer(w, rt) for w, rt in CALLS[name]]
    return _EXPECTED[name]


def _cast(a):
    return ctypes.cast(a, ctypes.c_void_p)


def _ptrs(tensors):
    return _cast((ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors]))


def _i64s(values):
    return _cast((ctypes.c_int64 * len(values))(*values))


def _poisoned(nbytes, dev):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)


def _check_zeroed(zero, count):
    """heads of the first `count` amax buffers are 0.0, every other byte is still 0xFF"""
    z = zero.cpu().numpy().view(np.uint32).reshape(-1, AMAX_FLOATS)
    want = np.full_like(z, 0xFFFFFFFF)
    want[:count, ::HEAD_STRIDE] = 0
    assert np.array_equal(z, want)


def _run(entry, layers, dev, zero_count=2):
    lib = _lib.load()
    n = len(layers)
    ws = [torch.from_numpy(w).to(dev) for w, _ in layers]
    rts = [None if rt is None else torch.from_numpy(rt).to(dev) for _, rt in layers]
    sizes = [packed_bytes(*w.shape) for w, _ in layers]
    for (w, _), sz in zip(layers, sizes):
        assert lib.rgcn_weights_split_bytes(*w.shape) == sz
    bufs = [_poisoned(sz, dev) for sz in sizes]
    zero = _poisoned((zero_count + 1) * AMAX_FLOATS * 4, dev).view(torch.float32)       # one buffer past the cleared ones
    dims = [_i64s([w.shape[k] for w, _ in layers]) for k in range(3)]
    csz = _cast((ctypes.c_size_t * n)(*sizes))
    stream = ops._stream()
    if entry == "absmax_pack":
        x = torch.linspace(-2, 1, 4 * 37 + 3, device=dev)
        x_amax = _poisoned(AMAX_FLOATS * 4, dev).view(torch.float32)
        rc = lib.rgcn_absmax_pack(x.data_ptr(), x.numel(), x_amax.data_ptr(), zero.data_ptr(), zero_count, n, _ptrs(ws),
                                  _ptrs(rts), *dims, _ptrs(bufs), csz, stream)
        _lib.check(rc, "rgcn_absmax_pack")
        _check_heads(x_amax, x.cpu().numpy())
        _check_zeroed(zero, zero_count)
    elif entry == "multi_scan":
        rc = lib.rgcn_weights_split_pack_multi(n, _ptrs(ws), _ptrs(rts), *dims, None, None, _ptrs(bufs), csz,
                                               zero.data_ptr(), zero_count, stream)
        _lib.check(rc, "rgcn_weights_split_pack_multi")
        _check_zeroed(zero, zero_count)
    elif entry == "multi_given":
        tensors = [t for pair in zip(ws, rts) for t in pair if t is not None]
        am = _poisoned(len(tensors) * AMAX_FLOATS * 4, dev).view(torch.float32).view(len(tensors), AMAX_FLOATS)
        rc = lib.rgcn_absmax_multi(len(tensors), _ptrs(tensors), _i64s([t.numel() for t in tensors]),
                                   _ptrs([am[k] for k in range(len(tensors))]), None, 0, stream)
        _lib.check(rc, "rgcn_absmax_multi")
        for k, t in enumerate(tensors):
            _check_heads(am[k], t.cpu().numpy().reshape(-1))
        wam, ram, k = [], [], 0
        for rt in rts:
            wam.append(am[k])
            ram.append(None if rt is None else am[k + 1])
            k += 1 if rt is None else 2
        rc = lib.rgcn_weights_split_pack_multi(n, _ptrs(ws), _ptrs(rts), *dims, _ptrs(wam), _ptrs(ram), _ptrs(bufs), csz,
                                               zero.data_ptr(), zero_count, stream)
        _lib.check(rc, "rgcn_weights_split_pack_multi")
        _check_zeroed(zero, zero_count)
    else:
        for w, rt, b, sz in zip(ws, rts, bufs, sizes):
            rc = lib.rgcn_weights_split_pack(w.data_ptr(), None if rt is None else rt.data_ptr(), *w.shape, b.data_ptr(), sz,
                                             stream)
            _lib.check(rc, "rgcn_weights_split_pack")
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in bufs]


def _check_heads(buf, values):
    """an amax buffer written into 0xFF bytes: every head holds a partial maximum, their maximum is max |values|, and
    nothing but the heads was touched"""
    a = buf.cpu().numpy().reshape(-1)
    heads = a[::HEAD_STRIDE]
    assert heads.shape == (HEADS,) and not np.isnan(heads).any() and (heads >= 0).all()
    want = np.abs(values).max() if values.size else np.float32(0)
    assert heads.max() == want, (heads.max(), want)
    rest = np.delete(a.view(np.uint32), np.arange(0, AMAX_FLOATS, HEAD_STRIDE))
    assert (rest == 0xFFFFFFFF).all()
    # head b: the maximum over the 1,024-float4 pieces b, b + 256, ... of the tensor (the tail, if any, with head 0)
    n4 = values.size // 4
    piece = (np.arange(n4 * 4) // 4096) % HEADS
    part = np.zeros(HEADS, dtype=np.float32)
    np.maximum.at(part, piece, np.abs(values[: n4 * 4]))
    if values.size > n4 * 4:
        part[0] = max(part[0], np.abs(values[n4 * 4:]).max())
    assert np.array_equal(heads, part)


def _compare(got, want, label):
    for k, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{label}, layer {k}: {bad.size} bytes differ, first at byte {bad[0]} of {g.size} "
                                 f"(got {g[bad[0]]:#x}, want {w[bad[0]]:#x})")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(CALLS))
def test_packed_bytes(name, entry):
    dev = need_gpu()
    _compare(_run(entry, CALLS[name], dev), _expected(name), f"{name} through {entry}")


@pytest.mark.parametrize("entry", ["multi_scan", "multi_given"])
def test_more_cleared_buffers_than_threads(entry):
    """zero_count up to 1,024 is accepted whatever the workgroup size of the launch"""
    dev = need_gpu()
    _compare(_run(entry, CALLS["c2_pair"], dev, zero_count=1024), _expected("c2_pair"), f"c2_pair through {entry}, 1,024 cleared")
    _compare(_run(entry, CALLS["one_tile"], dev, zero_count=300), _expected("one_tile"), f"one_tile through {entry}, 300 cleared")


def _x_cases():
    rng = np.random.default_rng(21)
    small = np.array([0.25, -3.0, 1.5, 0.5], dtype=np.float32)
    odd = rng.standard_normal(4 * 1500 + 3).astype(np.float32)
    odd[-1] = 9.0                                # the maximum in the tail past the last float4
    c2 = rng.standard_normal((30926, 64)).astype(np.float32)
    c2[-1, 17] = -11.0                           # the maximum in the last row
    return {"four": small, "tail": odd, "c2_last_row": c2.reshape(-1)}


X_CASES = _x_cases()


@pytest.mark.parametrize("entry", ["absmax", "absmax_pack"])
@pytest.mark.parametrize("case", list(X_CASES))
def test_x_scan(case, entry):
    dev = need_gpu()
    lib = _lib.load()
    values = X_CASES[case]
    x = torch.from_numpy(values).to(dev)
    x_amax = _poisoned(AMAX_FLOATS * 4, dev).view(torch.float32)
    zero = _poisoned(4 * AMAX_FLOATS * 4, dev).view(torch.float32)
    if entry == "absmax":
        _lib.check(lib.rgcn_absmax(x.data_ptr(), x.numel(), x_amax.data_ptr(), zero.data_ptr(), 3, ops._stream()), "rgcn_absmax")
    else:
        w, rt = CALLS["one_tile"][0]
        wd, rd = torch.from_numpy(w).to(dev), torch.from_numpy(rt).to(dev)
        sz = packed_bytes(*w.shape)
        buf = _poisoned(sz, dev)
        rc = lib.rgcn_absmax_pack(x.data_ptr(), x.numel(), x_amax.data_ptr(), zero.data_ptr(), 3, 1, _ptrs([wd]), _ptrs([rd]),
                                  _i64s([1]), _i64s([32]), _i64s([32]), _ptrs([buf]), _cast((ctypes.c_size_t * 1)(sz)),
                                  ops._stream())
        _lib.check(rc, "rgcn_absmax_pack")
        _compare([buf.cpu().numpy()], _expected("one_tile"), "one_tile beside the scan")
    _check_heads(x_amax, values)
    _check_zeroed(zero, 3)
