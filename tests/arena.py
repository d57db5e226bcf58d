"""Guard bands around caller-provided buffers: helper of tests/test_arena_host.py and tests/test_containment_gpu.py.

The suite checks what the kernels write INTO their outputs and workspaces.  A buffer from `torch.empty` sits inside a slab of the
caching allocator, so a store one element past its end lands in a neighbour or in free slab memory and nothing notices.  An `Arena` is
ONE uint8 allocation filled with 0xFF -- a NaN in bf16, fp16, fp32 and fp64, -1 as an integer -- that hands out typed views with
`band_bytes` of untouched arena on each side.  An overrun therefore lands in memory the test owns, and `check()` finds it.

    arena = Arena(device)                                   # or Arena(device, band_bytes, capacity_bytes)
    out = arena.take("out", numel, torch.bfloat16)          # 16-byte aligned
    odd = arena.take("factor", 3, torch.float16, offset_elems=1)   # 16-byte aligned plus one element
    ... launch, synchronise ...
    arena.check()                                           # every band byte is still 0xFF
    arena.assert_written("out")                             # no element of `out` still holds the poison pattern

`band_bytes` is a condition, not a measurement: at least 64 KiB, and at least the largest store footprint of one workgroup of the
entry under test (2048 elements of 8 bytes = 16 KiB for every kernel of this library), so that a workgroup that runs past the end of
its buffer cannot jump over the band.  Nothing here needs a GPU."""

from __future__ import annotations

from dataclasses import dataclass

import torch

POISON = 0xFF
MIN_BAND_BYTES = 64 * 1024
WORKGROUP_FOOTPRINT_BYTES = 2048 * 8  # the widest store footprint of one workgroup: a 2048-element chunk of fp64
ALIGN = 16


@dataclass(frozen=True)
class _View:
    name: str
    start: int  # byte offset of the view's first byte in the arena
    nbytes: int
    dtype: torch.dtype
    numel: int


class Arena:
    def __init__(self, device, band_bytes: int = MIN_BAND_BYTES, capacity_bytes: int = 32 << 20):
        if band_bytes < MIN_BAND_BYTES or band_bytes < WORKGROUP_FOOTPRINT_BYTES:
            raise ValueError(f"band_bytes = {band_bytes}: a band is at least {MIN_BAND_BYTES} bytes and at least one workgroup's store footprint ({WORKGROUP_FOOTPRINT_BYTES})")
        self.device, self.band_bytes = torch.device(device), int(band_bytes)
        self.buf = torch.full((int(capacity_bytes),), POISON, dtype=torch.uint8, device=self.device)
        if self.buf.data_ptr() % ALIGN:  # (torch's allocators align to 64 bytes and more; a typed view needs its byte offset to be a multiple of its element size)
            raise RuntimeError("the arena's allocation is not 16-byte aligned")
        self._views: dict[str, _View] = {}
        self._cursor = 0  # first byte no view or band has claimed

    def reset(self) -> None:
        "forget every view and poison the arena again (one allocation serves many cases)"
        self.buf.fill_(POISON)
        self._views.clear()
        self._cursor = 0

    def take(self, name: str, numel: int, dtype: torch.dtype, offset_elems: int = 0) -> torch.Tensor:
        """a view of `numel` elements of `dtype`, 16-byte aligned plus `offset_elems` elements (for the entries that accept any
        alignment), with `band_bytes` of arena nobody else is handed on each side"""
        if name in self._views:
            raise ValueError(f"the arena already holds a view called {name!r}")
        if numel < 0 or offset_elems < 0:
            raise ValueError("numel and offset_elems are not negative")
        size = torch.empty(0, dtype=dtype).element_size()
        aligned = self._cursor + self.band_bytes
        aligned += -aligned % ALIGN
        start, nbytes = aligned + offset_elems * size, numel * size
        end = start + nbytes + self.band_bytes
        if end > self.buf.numel():
            raise MemoryError(f"arena of {self.buf.numel()} bytes is full: {name!r} needs bytes up to {end}; pass a larger capacity_bytes")
        self._views[name] = _View(name, start, nbytes, dtype, numel)
        self._cursor = end
        view = self.buf[start : start + nbytes].view(dtype)
        assert (view.data_ptr() - offset_elems * size) % ALIGN == 0 and view.numel() == numel
        return view

    def view(self, name: str) -> torch.Tensor:
        v = self._views[name]
        return self.buf[v.start : v.start + v.nbytes].view(v.dtype)

    def check(self) -> None:
        "every band byte is still 0xFF; else names the buffer, the side, the first and last changed byte and how many changed"
        if not self._views:
            return
        # one pass over the used part of the arena decides; the bands are walked one by one only to describe a failure
        used = self.buf[: self._cursor]
        changed = used != POISON
        for v in self._views.values():
            changed[v.start : v.start + v.nbytes] = False
        if not bool(changed.any()):
            return
        found = []
        stray = changed.clone()  # what no band accounts for: the few bytes of alignment and element offset between one view's bands and the next one's
        for v in self._views.values():
            for side, lo, hi in (("before", v.start - self.band_bytes, v.start), ("after", v.start + v.nbytes, v.start + v.nbytes + self.band_bytes)):
                at = changed[lo:hi].nonzero().reshape(-1)
                stray[lo:hi] = False
                if at.numel():
                    first, last = int(at[0]), int(at[-1])
                    if side == "before":  # offsets relative to the view: -1 is the byte just in front of it
                        first, last = first - self.band_bytes, last - self.band_bytes
                    where = f"bytes {first} .. {last} " + ("in front of its first byte" if side == "before" else "past its end (0 = the first byte behind it)")
                    found.append(f"{v.name} ({v.numel} x {v.dtype}), band {side}: {at.numel()} byte(s) changed, {where}")
        at = stray.nonzero().reshape(-1)
        if at.numel():
            found.append(f"between the bands: {at.numel()} byte(s) changed, arena offsets {int(at[0])} .. {int(at[-1])}")
        raise AssertionError("stores outside a buffer:\n  " + "\n  ".join(found))

    def unwritten(self, name: str) -> torch.Tensor:
        "indices of the elements of view `name` that still hold the poison pattern (every byte 0xFF)"
        v = self._views[name]
        size = v.nbytes // v.numel if v.numel else 1
        raw = self.buf[v.start : v.start + v.nbytes].view(v.numel, size)
        return (raw == POISON).all(dim=1).nonzero().reshape(-1)

    def assert_written(self, name: str) -> None:
        "no element of that view still holds the poison pattern (outputs only: a workspace may be used in part)"
        left = self.unwritten(name)
        if left.numel():
            v = self._views[name]
            raise AssertionError(f"{name} ({v.numel} x {v.dtype}): {left.numel()} element(s) never written, the first at index {int(left[0])}, the last at {int(left[-1])}")


def untouched(t: torch.Tensor) -> bool:
    "every byte of this (contiguous) slice of an arena view is still poison"
    return bool((t.contiguous().view(torch.uint8) == POISON).all())
