"""CPU tier of the guard-band harness (``tests/guarded.py``): it must fail when it should.  The "kernel" here is a torch
write through an ``as_strided`` view that reaches outside the payload but stays inside the raw buffer the harness owns."""
import pytest
import torch

from guarded import BAND_BYTES, GuardedAllocator, bits, installed
from primekg_rgcn_linkprediction_amd import ops

CPU = torch.device("cpu")


def _stray_store(out: torch.Tensor, element: int, value=1.0) -> None:
    """store ``value`` at flat element index ``element`` of ``out``'s payload (negative: before it, >= numel: past it)"""
    out.as_strided((1,), (1,), out.storage_offset() + element).fill_(value)


def _raw(alloc: GuardedAllocator) -> torch.Tensor:
    return alloc.records[-1][4]


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_a_clean_kernel_passes_and_sees_the_fill(fill):
    alloc = GuardedAllocator(fill)
    out = alloc.empty(5, 7, dtype=torch.float32, device=CPU)
    assert torch.equal(out.view(torch.uint8), torch.full((5, 28), fill, dtype=torch.uint8))
    out.copy_(torch.arange(35.0).view(5, 7))                          # every element, nothing else
    alloc.check()
    assert alloc.damage() is None


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_one_element_past_the_end_is_detected(fill):
    alloc = GuardedAllocator(fill)
    alloc.empty(3, dtype=torch.int64, device=CPU)                     # allocation #0 stays clean
    out = alloc.empty(5, 7, dtype=torch.float32, device=CPU)
    _stray_store(out, 35)
    with pytest.raises(AssertionError) as err:
        alloc.check()
    msg = str(err.value)
    assert "allocation #1" in msg and "(5, 7)" in msg and "torch.float32" in msg
    # 1.0f = 00 00 80 3f: the pattern is never 0x00, so the first byte of the element differs
    assert "trailing band" in msg and "0 bytes past the payload's end" in msg


def test_one_element_before_the_start_is_detected():
    alloc = GuardedAllocator(0x00)
    out = alloc.empty((5, 7), dtype=torch.float32, device=CPU)
    _stray_store(out, -1)
    with pytest.raises(AssertionError) as err:
        alloc.check()
    msg = str(err.value)
    assert "allocation #0" in msg and "leading band" in msg and "4 bytes before the payload" in msg
    assert f"band byte {BAND_BYTES - 4}" in msg


@pytest.mark.parametrize("side", ["leading", "trailing"])
def test_the_far_edge_of_each_band_is_detected(side):
    alloc = GuardedAllocator(0xFF)
    out = alloc.empty(16, 4, dtype=torch.float32, device=CPU)
    words = BAND_BYTES // 4
    _stray_store(out, -words if side == "leading" else 64 + words - 1)
    with pytest.raises(AssertionError) as err:
        alloc.check()
    msg = str(err.value)
    assert f"{side} band" in msg
    assert ("band byte 0 " in msg) if side == "leading" else (f"band byte {BAND_BYTES - 4} " in msg)
    # and one element further would have left the raw buffer: the harness owns exactly band + payload + band
    assert _raw(alloc).numel() == 2 * BAND_BYTES + 256


def test_a_single_damaged_byte_of_a_byte_sized_payload_is_found_where_it_is():
    """an odd payload: the trailing band begins at the payload's last byte + 1, with no padding in between"""
    alloc = GuardedAllocator(0x00, band_bytes=512)
    out = alloc.empty(13, dtype=torch.uint8, device=CPU)
    raw = _raw(alloc)
    assert raw.numel() == 512 + 13 + 512 and out.data_ptr() == raw.data_ptr() + 512
    _stray_store(out, 13, 0)
    with pytest.raises(AssertionError, match="trailing band damaged at band byte 0 "):
        alloc.check()
    alloc = GuardedAllocator(0x00, band_bytes=512)
    out = alloc.empty(13, dtype=torch.uint8, device=CPU)
    _stray_store(out, 13 + 300, 0xFF)
    with pytest.raises(AssertionError, match=r"band byte 300 \(300 bytes past"):
        alloc.check()


def test_an_element_left_unwritten_differs_between_the_two_fills():
    want = torch.randn(6, 5, generator=torch.Generator().manual_seed(0))

    def kernel(out, skip):
        flat, src = out.view(-1), want.view(-1)
        for i in range(flat.numel()):
            if i != skip:
                flat[i] = src[i]
        return out

    results = {}
    for skip in (None, 17):
        for fill in (0x00, 0xFF):
            alloc = GuardedAllocator(fill)
            results[skip, fill] = kernel(alloc.empty(6, 5, dtype=torch.float32, device=CPU), skip)
            alloc.check()                                             # an unwritten element is no stray store
    assert torch.equal(bits(results[None, 0x00]), bits(results[None, 0xFF]))
    assert torch.equal(bits(results[None, 0x00]), bits(want))
    a, b = bits(results[17, 0x00]), bits(results[17, 0xFF])
    assert not torch.equal(a, b) and torch.nonzero(a != b).view(-1).tolist() == [17]
    # under 0xFF the element is a NaN: a value comparison that tolerates NaN would hide it, the bit pattern does not
    assert torch.isnan(results[17, 0xFF].view(-1)[17])


def test_bits_compares_patterns_not_values():
    nan_a = torch.tensor([0x7FC00000, 5], dtype=torch.int32).view(torch.float32)
    nan_b = torch.tensor([0x7FC00001, 5], dtype=torch.int32).view(torch.float32)
    assert torch.equal(bits(nan_a), bits(nan_a.clone())) and not torch.equal(bits(nan_a), bits(nan_b))
    assert not torch.equal(bits(torch.tensor([0.0])), bits(torch.tensor([-0.0])))
    assert bits(torch.zeros(3, dtype=torch.uint8)).dtype == torch.uint8          # 3 bytes: no int32 view
    assert bits(torch.zeros(3, dtype=torch.float16)).dtype == torch.uint8
    assert bits(torch.zeros(2, 3, dtype=torch.float64)).dtype == torch.int32
    assert bits(torch.zeros(0)).numel() == 0
    strided = torch.arange(12.0).view(3, 4).t()
    assert torch.equal(bits(strided), bits(strided.contiguous()))
    snap = torch.ones(4)
    kept = bits(snap)
    snap.add_(1.0)
    assert not torch.equal(kept, bits(snap))                                    # a snapshot, not a view


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.float64, torch.int32, torch.int64, torch.uint8])
def test_what_empty_returns_has_the_shape_dtype_and_alignment_of_torch_empty(dtype):
    alloc = GuardedAllocator(0xFF)
    for call, want in (((4, 3, 5), (4, 3, 5)), (((7, 9),), (7, 9)), ((torch.Size([2, 8]),), (2, 8)), ((33,), (33,))):
        out = alloc.empty(*call, dtype=dtype, device=CPU)
        ref = torch.empty(*call, dtype=dtype, device=CPU)
        raw = _raw(alloc)
        assert out.shape == ref.shape == torch.Size(want) and out.dtype == dtype and out.device == ref.device
        assert out.is_contiguous() and out.stride() == ref.stride()
        # the payload starts band_bytes (a multiple of 512) into the raw buffer: it is aligned as the raw buffer is
        assert out.data_ptr() - raw.data_ptr() == BAND_BYTES and BAND_BYTES % 512 == 0
        assert out.data_ptr() % 64 == 0 and out.data_ptr() % out.element_size() == 0
        assert raw.numel() == 2 * BAND_BYTES + out.numel() * out.element_size()
        assert bool((out.view(-1).view(torch.uint8) == 0xFF).all())
    assert [r[0] for r in alloc.records] == [0, 1, 2, 3]
    alloc.check()


@pytest.mark.parametrize("offset", [0, 16, 48, 496])
def test_the_payload_offset_moves_the_base_by_exactly_that_amount(offset):
    alloc = GuardedAllocator(0xFF, payload_offset=offset)
    plain = GuardedAllocator(0xFF)
    for shape, dtype in (((5, 7), torch.float32), ((13,), torch.uint8), ((3, 8), torch.float16), ((9,), torch.int64)):
        out, ref = alloc.empty(*shape, dtype=dtype, device=CPU), plain.empty(*shape, dtype=dtype, device=CPU)
        # torch's CPU allocator aligns to 64 bytes, the device allocator to 512 (asserted in the GPU tier): here the
        # move is measured against the start of the storage, a multiple of 64 with or without an offset
        base, ref_base = out.untyped_storage().data_ptr(), ref.untyped_storage().data_ptr()
        assert base % 64 == 0 and ref_base % 64 == 0
        assert (out.data_ptr() - base) - (ref.data_ptr() - ref_base) == offset and out.data_ptr() % 64 == offset % 64
        assert out.shape == ref.shape and out.dtype == ref.dtype and out.is_contiguous() and out.stride() == ref.stride()
        raw = _raw(alloc)
        # the record starts at the leading band: the bands sit directly around the payload, as without an offset
        assert out.data_ptr() - raw.data_ptr() == BAND_BYTES and raw.data_ptr() - base == offset
        assert raw.numel() == 2 * BAND_BYTES + out.numel() * out.element_size()
        assert bool((out.view(-1).view(torch.uint8) == 0xFF).all())
    alloc.check()
    assert alloc.damage() is None


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_bands_detect_strays_on_either_side_at_offset_16(fill):
    for element, side, where in ((-1, "leading", "4 bytes before the payload"), (35, "trailing", "0 bytes past the payload's end")):
        alloc = GuardedAllocator(fill, payload_offset=16)
        alloc.empty(3, dtype=torch.int64, device=CPU)                 # allocation #0 stays clean
        out = alloc.empty(5, 7, dtype=torch.float32, device=CPU)
        assert out.data_ptr() % 64 == 16
        out.copy_(torch.arange(35.0).view(5, 7))
        alloc.check()
        _stray_store(out, element)
        with pytest.raises(AssertionError) as err:
            alloc.check()
        msg = str(err.value)
        assert "allocation #1" in msg and f"{side} band" in msg and where in msg
    # the far edge of the leading band: the 16 bytes in front of it belong to the raw buffer, not to the band
    alloc = GuardedAllocator(fill, payload_offset=16)
    out = alloc.empty(16, 4, dtype=torch.float32, device=CPU)
    _stray_store(out, -(BAND_BYTES // 4))
    with pytest.raises(AssertionError, match="leading band damaged at band byte 0 "):
        alloc.check()


def test_an_unwritten_element_differs_between_the_fills_at_offset_16():
    want = torch.randn(6, 5, generator=torch.Generator().manual_seed(0))
    results = {}
    for fill in (0x00, 0xFF):
        alloc = GuardedAllocator(fill, payload_offset=16)
        out = alloc.empty(6, 5, dtype=torch.float32, device=CPU)
        assert out.data_ptr() % 64 == 16
        flat = out.view(-1)
        flat[:17] = want.view(-1)[:17]
        flat[18:] = want.view(-1)[18:]                                # element 17 is left as the allocator filled it
        alloc.check()
        results[fill] = bits(out)
    a, b = results[0x00], results[0xFF]
    assert torch.nonzero(a != b).view(-1).tolist() == [17]


def test_zero_size_requests_are_plain_tensors():
    alloc = GuardedAllocator(0x00)
    for call in ((0,), (0, 8), ((3, 0),), (torch.Size([0]),)):
        out = alloc.empty(*call, dtype=torch.float32, device=CPU)
        assert out.numel() == 0 and out.shape == torch.empty(*call).shape and out.dtype == torch.float32
    assert alloc.records == [] and alloc.calls == 4
    nxt = alloc.empty(2, dtype=torch.int32, device=CPU)
    assert alloc.records[0][0] == 4 and nxt.shape == (2,)             # call order counts every request
    alloc.check()


def test_bad_parameters_are_refused():
    with pytest.raises(ValueError):
        GuardedAllocator(0x5A)
    with pytest.raises(ValueError):
        GuardedAllocator(0x00, band_bytes=1000)
    for offset in (-16, 1, 4, 8, 24, BAND_BYTES, BAND_BYTES + 16):    # not a multiple of 16, or not inside the band
        with pytest.raises(ValueError, match="multiple of 16"):
            GuardedAllocator(0x00, payload_offset=offset)
    with pytest.raises(ValueError, match="multiple of 16"):
        GuardedAllocator(0x00, band_bytes=512, payload_offset=512)
    assert GuardedAllocator(0x00, band_bytes=512, payload_offset=496).payload_offset == 496


def test_installed_swaps_the_seam_and_puts_it_back(monkeypatch):
    before = ops._empty
    alloc = GuardedAllocator(0xFF)
    with installed(monkeypatch, alloc) as got:
        assert got is alloc and ops._empty == alloc.empty
        ws = ops._workspace(100, CPU)                                 # the library's own helper goes through the seam
        assert ws.numel() == 100 and len(alloc.records) == 1 and bool((ws == 0xFF).all())
        assert ops._workspace(0, CPU) is None
    assert ops._empty is before
    alloc.check()
    monkeypatch.setattr(ops, "_REC", object())
    with pytest.raises(AssertionError, match="Region"):
        with installed(monkeypatch, alloc):
            pass
    assert ops._empty is before
