"""Hostile memory for the launch paths: grids carved out of ONE poisoned allocation.

Every other test hands the engine whole, fresh torch allocations: 512-byte aligned, followed by allocator slack nobody
reads, the second buffer full of zeros.  ``carve`` gives it what a caller with one big allocation (or an exact-size
hipMalloc) gives it instead:

* every grid starts at an address that is 16 (mod 32) -- 16-byte aligned, the only promise of the C ABI
  (``check_buffers`` in capi.cpp), and provably no more; ``offset_bytes`` picks the phase inside a 512-byte block, so that
  the 64- and 128-byte lines the kernels' row pieces straddle fall differently;
* every byte before, between and after the grids is a GUARD band filled with a quiet NaN of a recognisable payload.  A store
  past a grid's end changes a guard byte (``assert_guards_intact``); a load past its end that reaches a result turns that
  result into NaN -- also through a zero tap -- and the bitwise comparison with the oracle fails.  Loads that are
  discarded cannot be seen this way and are not looked for.

The module works on CPU tensors too (tests/test_arena_helper.py shows there that it can fail).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

OFFSETS = (16, 48, 112, 240, 496)  # start address modulo 512; every one of them is 16 (mod 32)

# quiet NaNs with a payload nobody computes: fp64 0x7ff8dead0000beef, bf16 0x7fc1
POISON = {torch.float64: 0x7FF8DEAD0000BEEF, torch.bfloat16: 0x7FC1}
_INT = {torch.float64: torch.int64, torch.bfloat16: torch.int16}

# How far beyond a grid's end a wrong index of these kernels can reach -- the guard must hold it (detection ends where
# the guard ends).  From the kernel sources (lorastencil_amd/csrc):
#   2D  the tallest window any kernel stages is the single-sweep kernel's at rows_per_thread = 16: TH + 6 = 70 rows
#       (kernels_2d.hip: TH = 4 RPT, LH = TH + 6); the matrix-pipe kernel stages 40 (kernels_2d_mfma.hip: kLH), the tile
#       kernel fused_rows + 12 <= 22, the row-streaming and workgroup-row kernels keep at most stream_depth = 6 rows in
#       flight ahead of the row they consume; widest piece of a row: 520 doubles (kernels_2d_wg.hip: kBufW) -> 72 rows
#   3D  the z direction is streamed: one plane ahead in the register-resident kernels, a ring TWO planes ahead in the
#       plane-streaming, LDS-DMA and matrix-pipe kernels (kernels_3d_planes.hip, kernels_3d_bf16.hip: ring[3],
#       kernels_3d_bf16_mfma.hip: kDepth = 2) -> 4 planes; inside a plane the tallest tile is the bf16 register-resident
#       kernel's 16 waves x 4 rows = 64 rows of 128 columns (kernels_3d_bf16_lanes.hip) -> 72 rows, where a plane is less
#   1D  a workgroup's window is kFusedOut + 2 x 4 K = 1024 + 256 points at K = 32 (kernels_1d.hip) -> 4096 elements
GUARD_ROWS_2D = 72
GUARD_PLANES_3D = 4
GUARD_ROWS_3D = 72
GUARD_ELEMS_1D = 4096
GUARD_MIN_BYTES = 64 << 10


def torch_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        return dtype
    return {"f64": torch.float64, "fp64": torch.float64, "float64": torch.float64, "bf16": torch.bfloat16,
            "bfloat16": torch.bfloat16}[dtype]


def min_guard_bytes(padded_shape, dtype) -> int:
    """The least guard band for grids of this padded shape: the kernels' reach (above), never under 64 KiB."""
    item = torch.empty((), dtype=torch_dtype(dtype)).element_size()
    ps = tuple(int(x) for x in padded_shape)
    if len(ps) == 1:
        elems = GUARD_ELEMS_1D
    elif len(ps) == 2:
        elems = GUARD_ROWS_2D * ps[1]
    else:
        elems = max(GUARD_PLANES_3D * ps[1] * ps[2], GUARD_ROWS_3D * ps[2])
    return max(elems * item, GUARD_MIN_BYTES)


@dataclass
class Arena:
    flat: torch.Tensor            # the one allocation, as integers of the element size
    dtype: torch.dtype
    padded_shape: tuple
    views: list = field(default_factory=list)    # n_buffers tensors of `dtype` and `padded_shape`
    spans: list = field(default_factory=list)    # [(first element, one past the last)] of every view inside `flat`
    guards: list = field(default_factory=list)   # the same for the guard bands: before, between, after

    @property
    def poison(self) -> int:
        return POISON[self.dtype]

    @property
    def itemsize(self) -> int:
        return self.flat.element_size()

    def bits(self, i: int) -> torch.Tensor:
        """Integer view of buffer i (the way to compare NaNs)."""
        return self.views[i].view(_INT[self.dtype])

    def is_poison(self, i: int) -> torch.Tensor:
        return self.bits(i) == self.poison

    def fill_poison(self, i: int) -> None:
        self.bits(i).fill_(self.poison)


def carve(padded_shape, dtype, n_buffers: int = 2, offset_bytes: int = 16, guard_bytes: int | None = None,
          device="cuda") -> Arena:
    """One flat allocation full of poison; `n_buffers` contiguous views of `padded_shape`, each starting at an address
    that is `offset_bytes` (mod 512), guard bands of at least `guard_bytes` before, between and after them."""
    if offset_bytes not in OFFSETS:
        raise ValueError(f"offset_bytes must be one of {OFFSETS}")
    tdt = torch_dtype(dtype)
    idt = _INT[tdt]
    item = torch.empty((), dtype=tdt).element_size()
    ps = tuple(int(x) for x in padded_shape)
    need = min_guard_bytes(ps, tdt)
    guard_bytes = need if guard_bytes is None else int(guard_bytes)
    if guard_bytes < need:
        raise ValueError(f"guard bands of {guard_bytes} bytes do not hold the kernels' reach ({need})")
    count = int(np.prod(ps))
    nbytes = count * item
    # worst case per buffer: the guard, up to 512 bytes of phase adjustment, the grid
    total = n_buffers * (guard_bytes + 512 + nbytes) + guard_bytes + 512
    flat = torch.full(((total + item - 1) // item,), POISON[tdt], dtype=idt, device=device)
    base = flat.data_ptr()
    assert base % 16 == 0, "the allocator returned a block that is not even 16-byte aligned"
    arena = Arena(flat=flat, dtype=tdt, padded_shape=ps)
    pos = 0  # byte offset of the end of the previous buffer
    for _ in range(n_buffers):
        start = pos + guard_bytes
        start += (offset_bytes - (base + start)) % 512
        first = start // item
        view = flat[first:first + count].view(tdt).view(ps)
        assert view.data_ptr() == base + start and view.data_ptr() % 32 == 16 and view.is_contiguous()
        arena.views.append(view)
        arena.spans.append((first, first + count))
        arena.guards.append((pos // item, first))
        pos = start + nbytes
    arena.guards.append((pos // item, flat.numel()))
    assert flat.numel() * item - pos >= guard_bytes
    return arena


def guard_damage(arena: Arena) -> list:
    """[(band index, first touched byte, last touched byte, text)] of every guard band that no longer holds the poison;
    byte positions are offsets inside the arena."""
    item = arena.itemsize
    pattern = np.frombuffer(int(arena.poison).to_bytes(item, "little"), dtype=np.uint8)
    found = []
    for g, (lo, hi) in enumerate(arena.guards):
        band = arena.flat[lo:hi]
        if bool((band == arena.poison).all()):
            continue
        raw = band.cpu().numpy().view(np.uint8).reshape(-1, item)
        touched = np.flatnonzero((raw != pattern).ravel())
        first, last = lo * item + int(touched[0]), lo * item + int(touched[-1])

        def where(byte):
            # relative to the nearest edge of a buffer: end + k (k = 0: the first byte behind it) or start - k (k = 1:
            # the last byte in front of it)
            best = None
            for i, (b0, b1) in enumerate(arena.spans):
                for dist, text in ((byte - b1 * item, f"end of buffer {i} + {byte - b1 * item} bytes"),
                                   (b0 * item - byte, f"start of buffer {i} - {b0 * item - byte} bytes")):
                    if dist >= 0 and (best is None or dist < best[0]):
                        best = (dist, text)
            return best[1]

        found.append((g, first, last, f"guard band {g}: {len(touched)} bytes touched, first {where(first)}, "
                                      f"last {where(last)}"))
    return found


def assert_guards_intact(arena: Arena, what: str = "") -> None:
    damage = guard_damage(arena)
    assert not damage, (what + ": " if what else "") + "; ".join(d[3] for d in damage)
