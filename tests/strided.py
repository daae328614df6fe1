"""Operands of the C ABI (include/gwen_hip.h) at non-packed row pitches and member strides.

An ``Arena`` places every pitched operand of ONE call -- logical [members, rows, F] tensors, members possibly 1 -- in
ONE device allocation, each at its own (ld, mstride, base offset) with the tight extent
``(members-1)*mstride + (rows-1)*ld + F``.  Everything else in the allocation is padding: row padding, member gaps, a
lead-in before each base and a guard behind each operand's last element (at least 64 full pitches, and at least what
a kernel would cover if it took the packed stride for the pitched one or the other way round), so a wrong pitch lands
in memory the test owns.

    inputs   padding = the FINITE poison 2**100: kernels may load padding and mask it afterwards (0 * poison = 0 must
             not fail a test), but a padding value that is USED changes the bits of the result;
    outputs  the whole allocation, logical cells included, = a NaN with a fixed payload: an unwritten cell is visible,
             and so is a written padding cell.

``Arena.verify()`` is the checker: every logical output cell differs from the sentinel, and every other cell of the
allocation -- output padding, guards, the inputs and their padding -- is bit for bit (compared as int32) what it was
before the call.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

POISON = 2.0 ** 100
SENTINEL = 0x7FC5A5A5                 # a quiet NaN with a payload no kernel produces
LEAD = 64                             # floats before every operand's base (keeps the base 256-byte aligned + layout.base)


class Layout(NamedTuple):
    name: str
    ld: int
    mstride: int
    base: int                         # floats between a 16-byte aligned address and the first logical cell


LAYOUTS = ("packed", "row_pad", "member_gap", "window", "interleaved", "odd", "even")


def layout(name: str, members: int, rows: int, F: int, k: int = 1, j: int = 1) -> Layout:
    """The layouts of the stride tests by name.  ``even`` (8-byte aligned base, even pitch) is K2's two-wide path."""
    if name == "packed":
        return Layout(name, F, rows * F, 0)
    if name == "row_pad":
        return Layout(name, F + 4 * k, rows * (F + 4 * k), 0)
    if name == "member_gap":
        return Layout(name, F, rows * F + 4 * k, 0)
    if name == "window":
        ld = F + 4 * (j + k)
        return Layout(name, ld, rows * ld, 4 * j)
    if name == "interleaved":
        return Layout(name, members * F, F, 0)
    if name == "odd":
        return Layout(name, F + 1, rows * (F + 1) + 2, 1)
    if name == "even":
        return Layout(name, F + 2, rows * (F + 2) + 2, 2)
    raise KeyError(name)


class Operand:
    def __init__(self, arena, members, rows, F, lay, values, is_output):
        self.arena, self.members, self.rows, self.F, self.layout = arena, members, rows, F, lay
        self.ld, self.mstride, self.is_output = lay.ld, lay.mstride, is_output
        self._values = values
        self.extent = (members - 1) * lay.mstride + (rows - 1) * lay.ld + F
        # the furthest a kernel reaches that mixes up packed and pitched strides, or N and another row count
        wrong = members * max(rows * lay.ld, lay.mstride) + rows * lay.ld
        self.guard = max(64 * lay.ld, wrong - self.extent)
        self.offset = None             # of the first logical cell, in floats from the allocation's start

    @property
    def ptr(self) -> int:
        return self.arena.buf.data_ptr() + 4 * self.offset

    def _strided(self, t):
        return torch.as_strided(t, (self.members, self.rows, self.F), (self.mstride, self.ld, 1), self.offset)

    @property
    def view(self) -> torch.Tensor:
        """The logical [members, rows, F] tensor as a strided view of the allocation."""
        return self._strided(self.arena.buf)

    def values(self) -> torch.Tensor:
        return self.view.contiguous()


class Arena:
    """place operands -> commit() -> launch -> verify(); reset() puts the pre-call image back for a second launch."""

    def __init__(self, device="cuda:0"):
        self.device, self.ops, self.buf, self.total = torch.device(device), [], None, 0

    def _place(self, members, rows, F, lay, values, is_output):
        assert self.buf is None and lay.ld >= F and members >= 1 and rows >= 1 and F >= 1
        op = Operand(self, members, rows, F, lay, values, is_output)
        start = (self.total + 63) // 64 * 64
        op.offset = start + LEAD + lay.base
        self.total = op.offset + op.extent + op.guard
        self.ops.append(op)
        return op

    def input(self, values: torch.Tensor, lay: Layout) -> Operand:
        v = values if values.dim() == 3 else values.unsqueeze(0)
        return self._place(v.size(0), v.size(1), v.size(2), lay, v, False)

    def output(self, members: int, rows: int, F: int, lay: Layout) -> Operand:
        return self._place(members, rows, F, lay, None, True)

    def commit(self):
        has_out = any(o.is_output for o in self.ops)
        self.buf = torch.empty(self.total + 64, dtype=torch.float32, device=self.device)
        assert self.buf.data_ptr() % 16 == 0
        bits = self.buf.view(torch.int32)
        if has_out:
            bits.fill_(SENTINEL)
        self.logical_out = torch.zeros(self.buf.numel(), dtype=torch.bool, device=self.device)
        lo = 0
        for o in self.ops:
            hi = o.offset + o.extent + o.guard
            if o.is_output:
                bits[lo:hi].fill_(SENTINEL)
                cells = o._strided(self.logical_out)
                assert not bool(cells.any()), "two logical cells coincide"
                cells.fill_(True)
            else:
                self.buf[lo:hi].fill_(POISON)
                o.view.copy_(o._values.to(self.device))
                assert torch.equal(o.view, o._values.to(self.device)), "two logical cells coincide"
            lo = hi
        if not has_out:
            self.buf[lo:].fill_(POISON)
        self.before = bits.clone()
        return self

    def reset(self):
        self.buf.view(torch.int32).copy_(self.before)

    def verify(self, what=""):
        """Both jobs of the checker, after the launch (synchronises)."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        bits = self.buf.view(torch.int32)
        same = bits == self.before
        unwritten = int((same & self.logical_out).sum())           # logical cells still hold the sentinel
        assert unwritten == 0, f"{what}: {unwritten} logical output cells were never written"
        touched = ~same & ~self.logical_out
        if bool(touched.any()):
            where = torch.nonzero(touched).flatten()[:8].tolist()
            owner = [(o.layout.name, "out" if o.is_output else "in", o.offset) for o in self.ops]
            raise AssertionError(f"{what}: {int(touched.sum())} cells outside the logical outputs changed "
                                 f"(padding, guard or an input), first at float offsets {where}; operands {owner}")
