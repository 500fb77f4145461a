"""tests/arena.py on CPU tensors: the helper the GPU memory-contract tests stand on must itself be able to fail."""
import numpy as np
import pytest
import torch

import arena as A

CASES = [((1032,), "f64"), ((41, 138), "f64"), ((9, 12, 70), "f64"), ((11, 25, 272), "bf16")]


@pytest.mark.parametrize("ps,dtype", CASES)
@pytest.mark.parametrize("offset", A.OFFSETS)
def test_carved_pointers_are_16_byte_aligned_and_no_more(ps, dtype, offset):
    ar = A.carve(ps, dtype, n_buffers=3, offset_bytes=offset, device="cpu")
    assert len(ar.views) == 3
    for v in ar.views:
        ptr = v.data_ptr()
        assert ptr % 16 == 0 and ptr % 32 == 16
        assert ptr % 512 == offset
        assert tuple(v.shape) == ps and v.is_contiguous() and v.dtype == A.torch_dtype(dtype)
    A.assert_guards_intact(ar)


@pytest.mark.parametrize("ps,dtype", CASES)
def test_views_and_guards_tile_the_arena_without_overlap(ps, dtype):
    ar = A.carve(ps, dtype, n_buffers=2, offset_bytes=112, device="cpu")
    item = ar.itemsize
    base = ar.flat.data_ptr()
    pieces = sorted([(lo, hi, "guard") for lo, hi in ar.guards] + [(lo, hi, "view") for lo, hi in ar.spans])
    assert pieces[0][0] == 0 and pieces[-1][1] == ar.flat.numel()
    for (lo0, hi0, k0), (lo1, hi1, k1) in zip(pieces[:-1], pieces[1:]):
        assert hi0 == lo1 and k0 != k1  # back to back, guard / view / guard / ...
    assert [k for _, _, k in pieces] == ["guard", "view", "guard", "view", "guard"]
    for v, (lo, hi) in zip(ar.views, ar.spans):
        assert v.data_ptr() == base + lo * item and hi - lo == v.numel()
    # every guard band holds the kernels' reach: the floor, and the rows / planes / elements of the shape
    need = A.min_guard_bytes(ps, dtype)
    assert need >= 64 << 10
    row = ps[-1] * item
    if len(ps) == 2:
        assert need >= 8 * row
    elif len(ps) == 3:
        assert need >= 2 * ps[1] * row
    else:
        assert need >= 4096 * item
    for lo, hi in ar.guards:
        assert (hi - lo) * item >= need
    with pytest.raises(ValueError):
        A.carve(ps, dtype, guard_bytes=need - 16, device="cpu")
    with pytest.raises(ValueError):
        A.carve(ps, dtype, offset_bytes=32, device="cpu")
    # writing every cell of every view leaves the guards alone; the views start as poison
    for i, v in enumerate(ar.views):
        assert bool(ar.is_poison(i).all()) and bool(torch.isnan(v.double()).all())
        v.fill_(1.0)
        assert not bool(ar.is_poison(i).any())
    A.assert_guards_intact(ar)


@pytest.mark.parametrize("ps,dtype", CASES)
def test_a_planted_byte_in_each_guard_band_is_reported(ps, dtype):
    ar = A.carve(ps, dtype, n_buffers=2, offset_bytes=48, device="cpu")
    item = ar.itemsize
    raw = ar.flat.view(torch.uint8)
    assert len(ar.guards) == 3
    for g, (lo, hi) in enumerate(ar.guards):
        # the first byte of the band, its last byte, and one in the middle: one byte, one bit
        for byte in (lo * item, hi * item - 1, (lo + hi) // 2 * item + item // 2):
            keep = int(raw[byte])
            raw[byte] = keep ^ 0x01
            damage = A.guard_damage(ar)
            assert [(d[0], d[1], d[2]) for d in damage] == [(g, byte, byte)]
            with pytest.raises(AssertionError) as e:
                A.assert_guards_intact(ar, "planted")
            text = str(e.value)
            assert f"guard band {g}" in text and "1 bytes touched" in text
            if byte == lo * item and g > 0:
                assert f"end of buffer {g - 1} + 0 bytes" in text
            if byte == hi * item - 1 and g < 2:
                assert f"start of buffer {g} - 1 bytes" in text
            raw[byte] = keep
            A.assert_guards_intact(ar)
    # a touched range: first and last offset are both named
    lo, hi = ar.guards[1]
    raw[lo * item + 8] = 0
    raw[lo * item + 200] = 0
    (d,) = A.guard_damage(ar)
    assert (d[1], d[2]) == (lo * item + 8, lo * item + 200)
    assert "end of buffer 0 + 8 bytes" in d[3] and "end of buffer 0 + 200 bytes" in d[3]


def test_poison_is_a_quiet_nan_that_survives_a_zero_tap():
    for dtype, bits in ((torch.float64, np.array([A.POISON[torch.float64]], dtype=np.uint64).view(np.float64)),
                        (torch.bfloat16, (np.array([A.POISON[torch.bfloat16]], dtype=np.uint32) << 16).view(np.float32))):
        assert np.isnan(bits[0]) and np.isnan(bits[0] * 0.0)
    ar = A.carve((16,), "f64", device="cpu")
    assert int(ar.bits(0)[0]) == 0x7FF8DEAD0000BEEF
    ar = A.carve((3, 6, 16), "bf16", device="cpu")
    assert int(ar.bits(0)[0, 0, 0]) == 0x7FC1
