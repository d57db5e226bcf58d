"""tests/arena.py on CPU tensors: the guard bands catch a planted store on either side of a view, assert_written catches one element
left alone in every dtype, and a clean arena passes.  Without this the GPU module (tests/test_containment_gpu.py) could pass vacuously."""

import pytest
import torch

from arena import MIN_BAND_BYTES, POISON, Arena, untouched

DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.float64]
CAPACITY = 1 << 20


def filled(arena: Arena, name: str, numel: int, dtype, offset_elems: int = 0) -> torch.Tensor:
    t = arena.take(name, numel, dtype, offset_elems)
    t.copy_(torch.arange(numel, dtype=torch.float32).to(dtype))
    return t


def test_poison_is_a_nan_in_every_dtype_and_views_are_placed_as_documented():
    arena = Arena("cpu", capacity_bytes=2 * CAPACITY)
    for i, dtype in enumerate(DTYPES):
        size = torch.empty(0, dtype=dtype).element_size()
        a = arena.take(f"a{i}", 37, dtype)
        b = arena.take(f"b{i}", 5, dtype, offset_elems=1)
        assert a.dtype == dtype and a.numel() == 37 and torch.isnan(a).all() and torch.isnan(b).all()
        assert a.data_ptr() % 16 == 0 and (b.data_ptr() - size) % 16 == 0 and b.data_ptr() % 16 != 0
        assert b.data_ptr() - (a.data_ptr() + 37 * size) >= 2 * MIN_BAND_BYTES  # a band behind `a` and another in front of `b`
        assert untouched(a) and untouched(b[1:3])
    ints = arena.take("ints", 4, torch.int32)
    assert ints.tolist() == [-1] * 4
    assert arena.view("a0").data_ptr() == arena.buf.data_ptr() + MIN_BAND_BYTES
    with pytest.raises(ValueError):
        arena.take("ints", 1, torch.int32)
    with pytest.raises(MemoryError):
        arena.take("too much", CAPACITY, torch.uint8)
    with pytest.raises(ValueError):
        Arena("cpu", band_bytes=MIN_BAND_BYTES - 1, capacity_bytes=CAPACITY)


@pytest.mark.parametrize("offset_elems", [0, 1])
def test_a_clean_arena_passes(offset_elems):
    arena = Arena("cpu", capacity_bytes=CAPACITY)
    arena.check()  # nothing handed out yet
    for i, dtype in enumerate(DTYPES):
        filled(arena, f"v{i}", 2048 + 3, dtype, offset_elems)
    filled(arena, "empty", 0, torch.float32)
    arena.check()
    for i in range(len(DTYPES)):
        arena.assert_written(f"v{i}")
    arena.assert_written("empty")
    arena.reset()
    assert bool((arena.buf == POISON).all())
    filled(arena, "v0", 5, torch.float64)  # the name is free again
    arena.check()


@pytest.mark.parametrize("offset_elems", [0, 1])
def test_check_catches_one_byte_just_before_a_view(offset_elems):
    arena = Arena("cpu", capacity_bytes=CAPACITY)
    filled(arena, "neighbour_a", 8, torch.float32)
    v = filled(arena, "victim", 37, torch.bfloat16, offset_elems)
    filled(arena, "neighbour_b", 8, torch.float64)
    at = v.data_ptr() - arena.buf.data_ptr() - 1
    arena.buf[at] = 0x7F
    with pytest.raises(AssertionError) as err:
        arena.check()
    text = str(err.value)
    assert "victim (37 x torch.bfloat16), band before: 1 byte(s) changed, bytes -1 .. -1" in text
    assert "neighbour" not in text
    arena.buf[at] = POISON
    arena.check()


@pytest.mark.parametrize("offset_elems", [0, 1])
def test_check_catches_one_byte_just_after_a_view(offset_elems):
    arena = Arena("cpu", capacity_bytes=CAPACITY)
    filled(arena, "neighbour_a", 8, torch.float32)
    v = filled(arena, "victim", 105, torch.float64, offset_elems)
    filled(arena, "neighbour_b", 8, torch.float16)
    at = v.data_ptr() - arena.buf.data_ptr() + 105 * 8
    arena.buf[at] = 0
    with pytest.raises(AssertionError) as err:
        arena.check()
    text = str(err.value)
    assert "victim (105 x torch.float64), band after: 1 byte(s) changed, bytes 0 .. 0" in text
    assert "neighbour" not in text
    arena.buf[at] = POISON
    arena.check()


def test_check_reports_the_extent_of_an_overrun_and_the_far_end_of_a_band():
    arena = Arena("cpu", capacity_bytes=CAPACITY)
    v = filled(arena, "slots", 4, torch.float64)
    end = v.data_ptr() - arena.buf.data_ptr() + 32
    arena.buf[end : end + 16] = 0  # a pair of doubles written into slot `n_slots`
    arena.buf[end + MIN_BAND_BYTES - 1] = 1  # and the last byte the band owns
    with pytest.raises(AssertionError) as err:
        arena.check()
    assert f"slots (4 x torch.float64), band after: 17 byte(s) changed, bytes 0 .. {MIN_BAND_BYTES - 1}" in str(err.value)


def test_check_describes_a_changed_byte_in_the_gap_between_two_views_bands():
    "the alignment and element offset of a view leave a few bytes that belong to no band: a store there is still located"
    arena = Arena("cpu", capacity_bytes=CAPACITY)
    a = filled(arena, "odd", 5, torch.bfloat16)  # 10 bytes: the next view's 16-byte alignment leaves a gap
    b = filled(arena, "next", 4, torch.float64, offset_elems=1)
    gap = a.data_ptr() - arena.buf.data_ptr() + 10 + MIN_BAND_BYTES  # the first byte behind the band of `odd`
    assert gap < b.data_ptr() - arena.buf.data_ptr() - MIN_BAND_BYTES  # and in front of the band of `next`
    arena.buf[gap] = 3
    with pytest.raises(AssertionError) as err:
        arena.check()
    assert f"between the bands: 1 byte(s) changed, arena offsets {gap} .. {gap}" in str(err.value) and "band before" not in str(err.value)
    arena.buf[gap] = POISON
    arena.check()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hole", [0, 17, 36])
def test_assert_written_catches_a_single_element_left_unwritten(dtype, hole):
    arena = Arena("cpu", capacity_bytes=CAPACITY)
    v = arena.take("out", 37, dtype, offset_elems=1)
    keep = torch.arange(37) != hole
    v[keep] = torch.randn(36).to(dtype)
    arena.check()  # the bands are clean: only the output is incomplete
    assert arena.unwritten("out").tolist() == [hole]
    with pytest.raises(AssertionError) as err:
        arena.assert_written("out")
    assert f"1 element(s) never written, the first at index {hole}" in str(err.value)
    v[hole] = 0.0
    arena.assert_written("out")
