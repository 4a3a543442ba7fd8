"""A byte arena that hands out launch workspaces in place of `engine._workspace`, each between two canaries.

Layout of one hand-out, back to back from the arena's 256-aligned base:

    [head canary 256 B][workspace: exactly the bytes asked for][tail canary 4096 B][pad to the next multiple of 256]

The workspace starts 256-aligned (the entries need 16), the tail canary starts at the first byte behind it.  The arena never
allocates after its construction, so the same sequence of hand-outs lands on the same bytes: that is what `keep()` relies on to
present a launch with what an earlier launch left behind.  Works on a CPU tensor as well (tests/test_workspace_arena_cpu.py).
"""
from typing import List, Optional, Tuple

import torch

HEAD = 256
TAIL = 4096
ALIGN = 256
CANARY = 0xA5
MIN_BYTES = 256        # engine._workspace never returns less


class CanaryDamage(AssertionError):
    """`offset` = the first damaged byte relative to the END of its workspace: 0 is the first byte behind it, -(length + 1) the
    last byte in front of it; `handout` = its index since the last reset."""

    def __init__(self, handout: int, length: int, offset: int, value: int):
        self.handout, self.length, self.offset, self.value = handout, length, offset, value
        side = "behind the end" if offset >= 0 else "before the start"
        at = offset if offset >= 0 else -offset - length
        super().__init__(f"hand-out {handout} ({length} bytes): byte {at} {side} of the workspace holds 0x{value:02X}, not 0x{CANARY:02X} "
                         f"(offset {offset} from the workspace's end)")


def _up(v: int, a: int) -> int:
    return (v + a - 1) // a * a


class WorkspaceArena:
    def __init__(self, capacity: int, device="cpu"):
        self.device = torch.device(device)
        self._raw = torch.empty(int(capacity) + ALIGN, dtype=torch.uint8, device=self.device)
        base = -self._raw.data_ptr() % ALIGN                  # a device allocation is 256-aligned already, a host one need not be
        self.buf = self._raw[base:base + int(capacity)]
        self.handouts: List[Tuple[int, int]] = []             # (offset of the workspace in buf, its length) since the last reset
        self._cursor = 0
        self.fill(0)

    # ------------------------------------------------------------------ hand-outs
    def slice(self, n_bytes: int, device=None) -> torch.Tensor:
        """the next workspace of exactly n_bytes, its canaries freshly set; whatever the bytes held before stays"""
        n = int(n_bytes)
        assert n >= 1
        assert device is None or self._same_device(device), (device, self.device)
        off = self._cursor + HEAD
        end = off + n + TAIL
        assert end <= self.buf.numel(), f"arena of {self.buf.numel()} bytes is too small for a hand-out that ends at {end}"
        self.buf[off - HEAD:off] = CANARY
        self.buf[off + n:end] = CANARY
        self.handouts.append((off, n))
        self._cursor = _up(end, ALIGN)
        return self.buf[off:off + n]

    def workspace(self, n_bytes: int, device=None) -> torch.Tensor:
        """drop-in for engine._workspace: max(n_bytes, 256) bytes"""
        return self.slice(max(int(n_bytes), MIN_BYTES), device)

    def _same_device(self, device) -> bool:
        d = torch.device(device)
        return d.type == self.device.type and (d.index is None or self.device.index is None or d.index == self.device.index)

    # ------------------------------------------------------------------ states
    def reset(self) -> None:
        """forget the hand-outs; the bytes stay"""
        self.handouts = []
        self._cursor = 0

    def keep(self) -> None:
        """the next hand-outs start over at the arena's base and find the bytes as they are now: the leftovers of whatever ran"""
        self.reset()

    def _restore(self) -> None:
        for off, n in self.handouts:
            self.buf[off - HEAD:off] = CANARY
            self.buf[off + n:off + n + TAIL] = CANARY

    def fill(self, byte: int) -> None:
        """every workspace byte (handed out or not yet) = byte; the canaries of the recorded hand-outs are put back"""
        self.buf.fill_(int(byte))
        self._restore()

    def fill_random(self, seed: int) -> None:
        g = torch.Generator(device="cpu")
        g.manual_seed(int(seed))
        n = self.buf.numel()
        words = torch.randint(-2 ** 63, 2 ** 63 - 1, (_up(n, 8) // 8,), dtype=torch.int64, generator=g)
        self.buf.copy_(words.view(torch.uint8)[:n])
        self._restore()

    # ------------------------------------------------------------------ the check
    def damage(self) -> Optional[CanaryDamage]:
        for i, (off, n) in enumerate(self.handouts):
            for lo, hi in ((off - HEAD, off), (off + n, off + n + TAIL)):
                bad = (self.buf[lo:hi] != CANARY).nonzero()
                if bad.numel():
                    pos = lo + int(bad[0, 0])
                    return CanaryDamage(i, n, pos - (off + n), int(self.buf[pos]))
        return None

    def check(self) -> None:
        """every canary byte of every hand-out since the last reset still holds 0xA5 (synchronise the device before)"""
        d = self.damage()
        if d is not None:
            raise d
