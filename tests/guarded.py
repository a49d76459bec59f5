"""Guard bands and poison fills for every tensor the library is handed (``tests/test_guarded.py``, and
``tests/test_guarded_host.py`` for the harness itself).  A plain module, not a conftest.

The GPU tier compares values, and values do not show a store one row past a ragged tile (it lands in the caching
allocator's slack or in a neighbour) nor a read of memory no kernel wrote (it is whatever the block held last).  Every
allocation of the library's wrappers goes through ``ops._empty``; ``GuardedAllocator.empty`` stands in for it and
returns the payload of ``[band | payload | band]``: the bands hold a fixed byte pattern that ``check()`` compares
bit for bit, the payload is pre-filled with ``0x00`` or ``0xFF`` so that a result which depends on unwritten memory
differs between a run under the one fill and a run under the other.

The band is 1 MiB on each side: a CONDITION on the scenarios, not a measurement - their output rows are at most 8 KiB,
so a store at a row index up to 127 past either end of any output stays inside memory this module owns.  The harness
itself only ever writes inside its own buffers.
"""
import contextlib

import torch

BAND_BYTES = 1 << 20


def _pattern(nbytes: int, device) -> torch.Tensor:
    """the bands' bytes: position dependent, never 0x00 and never 0xFF (neither fill, nor a cleared word)"""
    i = torch.arange(nbytes, dtype=torch.int64, device=device)
    return ((i * 131 + 17) % 251 + 2).to(torch.uint8)


def bits(t: torch.Tensor) -> torch.Tensor:
    """the bit pattern of ``t`` as a flat integer tensor (int32 where the element size allows, else uint8): two
    tensors hold the same bits iff ``torch.equal(bits(a), bits(b))`` - NaN payloads and signed zeros included (the
    order of the bytes inside a word does not matter here, only that the pattern is compared exactly)"""
    flat = t.detach().contiguous().reshape(-1)
    if flat.numel() == 0:
        return torch.empty(0, dtype=torch.uint8, device=flat.device)
    return flat.view(torch.int32 if (flat.numel() * flat.element_size()) % 4 == 0 else torch.uint8).clone()


class GuardedAllocator:
    """``empty`` with ``ops._empty``'s signature; every raw buffer is kept until ``check()`` has looked at it"""

    def __init__(self, fill: int, band_bytes: int = BAND_BYTES, payload_offset: int = 0):
        """``payload_offset``: the payload (and the bands around it) start that many bytes later, so a payload begins
        ``payload_offset`` bytes past a 512-byte boundary instead of on one - the smallest base the 16-byte contract of
        ``include/rgcn_hip.h`` allows is 16.  0: the payload keeps ``torch.empty``'s alignment."""
        if fill not in (0x00, 0xFF):
            raise ValueError("fill must be 0x00 or 0xFF")
        if band_bytes <= 0 or band_bytes % 512:
            raise ValueError("band_bytes must be a positive multiple of 512 (the payload keeps torch.empty's alignment)")
        if payload_offset < 0 or payload_offset % 16 or payload_offset >= band_bytes:
            raise ValueError("payload_offset must be a multiple of 16 (the alignment every entry point accepts), "
                             "at least 0 and smaller than the band")
        self.fill, self.band_bytes, self.payload_offset = fill, band_bytes, payload_offset
        self.records = []                     # (call order, shape, dtype, payload bytes, raw uint8 buffer)
        self.calls = 0                        # every request, zero-size ones included
        self._patterns = {}

    def _band(self, device) -> torch.Tensor:
        key = str(device)
        if key not in self._patterns:
            self._patterns[key] = _pattern(self.band_bytes, device)
        return self._patterns[key]

    def empty(self, *shape, dtype, device) -> torch.Tensor:
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        shape = tuple(int(s) for s in shape)
        order = self.calls
        self.calls += 1
        numel = 1
        for s in shape:
            numel *= s
        if numel == 0:
            return torch.empty(shape, dtype=dtype, device=device)
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        band = self.band_bytes
        # [offset bytes nobody looks at | band | payload | band]: the record is the part from the leading band on
        raw = torch.empty(self.payload_offset + band + nbytes + band, dtype=torch.uint8, device=device)[self.payload_offset:]
        pattern = self._band(raw.device)
        raw[:band] = pattern
        raw[band:band + nbytes] = self.fill
        raw[band + nbytes:] = pattern                        # begins at the payload's last byte + 1: no padding
        self.records.append((order, shape, dtype, nbytes, raw))
        return raw[band:band + nbytes].view(dtype).view(shape)

    def damage(self):
        """-> None, or the description of the first damaged band byte (allocations in call order, leading band first)"""
        band = self.band_bytes
        for order, shape, dtype, nbytes, raw in self.records:
            pattern = self._band(raw.device)
            for side, lo in (("leading", 0), ("trailing", band + nbytes)):
                got = raw[lo:lo + band]
                if torch.equal(got, pattern):
                    continue
                at = int(torch.nonzero(got != pattern)[0])
                where = f"{band - at} bytes before the payload" if side == "leading" else f"{at} bytes past the payload's end"
                return (f"allocation #{order} (shape {shape}, {dtype}, {nbytes} payload bytes): {side} band damaged at "
                        f"band byte {at} ({where}): holds 0x{int(got[at]):02x}, was 0x{int(pattern[at]):02x}")
        return None

    def check(self) -> None:
        """assert that every band of every allocation so far is bit-intact"""
        found = self.damage()
        assert found is None, found


@contextlib.contextmanager
def installed(monkeypatch, alloc: GuardedAllocator):
    """``ops._empty = alloc.empty`` for the body (no ``Region`` may be recording: its arena is not guarded)"""
    from primekg_rgcn_linkprediction_amd import ops
    assert ops._REC is None, "a Region is recording: its allocations come from the pass's arena"
    with monkeypatch.context() as m:
        m.setattr(ops, "_empty", alloc.empty)
        yield alloc
        assert ops._REC is None
