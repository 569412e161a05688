"""An arena with checked flanks (TEST INFRASTRUCTURE): where a kernel writes, not what it computes.

The value tests hand the library tensors that torch allocated; the caching allocator rounds those up and parks other live
tensors beside them, so a kernel that stores one pack, one tile column, one status byte or one digest past its output damages
memory no assertion looks at.  An ``Arena`` is ONE uint8 allocation filled with a position-dependent pattern.  A test reserves
its operands and outputs as *windows* of it -- each at a chosen alignment phase, each with a flank of pattern bytes before and
after it (at least as long as the window, never shorter than 64 KiB), matrix rows a pitch apart with the gaps left as pattern --
hands the raw pointers to the C ABI and then calls ``check()``:

* every byte outside an ``out`` / ``inout`` window still equals the pattern (flanks, row gaps, unused space), and
* every ``in`` window still holds what was loaded into it.

Every flank lies inside the one allocation, so an overrun is a failed assertion and never a fault.  The pattern (``pattern``):
aligned 8-byte word i is (i + 1) * 0x9E3779B97F4A7C15 mod 2^64, with every byte that came out 0, 1, 2 or 0xFF flipped by 0x5A.
No word is 0 or all-ones, no word equals its neighbour (a kernel that stores a constant, or copies a flank word onto the next,
does not pass), and no byte is one of the status / verdict values the library writes.  Works on "cpu" as well: the self-tests of
tests/test_redzone_model.py run without a GPU.
"""
from __future__ import annotations

import numpy as np
import torch

MIN_FLANK = 64 * 1024
DEFAULT_CAPACITY = 8 << 20
MAX_CAPACITY = 16 << 20     # the longest fill whose word properties tests/test_redzone_model.py checks
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
KINDS = ("in", "out", "inout")
_PRISTINE = {}


def pattern(nbytes: int) -> np.ndarray:
    """the first nbytes of the fill, as uint8"""
    words = (nbytes + 7) // 8
    with np.errstate(over="ignore"):
        w = np.arange(1, words + 1, dtype=np.uint64) * _GOLDEN
    b = w.view(np.uint8)
    b[(b <= 2) | (b == 255)] ^= np.uint8(0x5A)
    return b[:nbytes]


class RedZoneError(AssertionError):
    """check() failed.  ``strays``: one dict per (window, side) that was hit -- window, side ("before", "after", "gap",
    "inside"), offset (of the stray byte nearest the window's edge), row, count; ``count``: all differing bytes."""

    def __init__(self, message, strays, count):
        super().__init__(message)
        self.strays = strays
        self.count = count


class Window:
    """rows x nbytes bytes of the arena, rows `pitch` bytes apart.  ``ptr`` is the raw device address of the first byte (for
    ctypes); ``view`` a uint8 [rows][nbytes] tensor over the same memory."""

    def __init__(self, arena, name, kind, start, nbytes, rows, pitch):
        self.arena, self.name, self.kind = arena, name, kind
        self.start, self.nbytes, self.rows, self.pitch = start, nbytes, rows, pitch
        self.end = start + (rows - 1) * pitch + nbytes        # one past the last byte
        self.ptr = arena.base + start
        self.view = torch.as_strided(arena.data, (rows, nbytes), (pitch, 1), start)

    def load(self, a):
        """fill the window from a numpy array (any dtype; rows * nbytes bytes, row-major without the pitch).  For an `in`
        window this is what check() expects to find afterwards."""
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(self.rows, self.nbytes)
        t = torch.from_numpy(raw.copy()).to(self.arena.data.device)
        self.view.copy_(t)
        if self.kind == "in":
            torch.as_strided(self.arena.expect, (self.rows, self.nbytes), (self.pitch, 1), self.start).copy_(t)
        return self

    def read(self, dtype=np.uint8) -> np.ndarray:
        """the window's bytes on the host, [rows][nbytes / itemsize]"""
        self.arena.sync()
        return np.ascontiguousarray(self.view.cpu().numpy()).view(dtype)

    def locate(self, p):
        """(side, offset, row) of arena byte p relative to this window; the distance to the window is abs(offset) outside it"""
        if p < self.start:
            return "before", p - self.start, 0                 # -1: the byte just before the window
        if p >= self.end:
            return "after", p - self.end + 1, self.rows - 1    # +1: the byte just after it
        row, col = divmod(p - self.start, self.pitch)
        if col < self.nbytes:
            return "inside", col, row
        return "gap", col - self.nbytes + 1, row               # +1: the first gap byte after row `row`


class Arena:
    def __init__(self, device="cuda", capacity=DEFAULT_CAPACITY):
        assert capacity <= MAX_CAPACITY, "the fill's word properties are checked up to MAX_CAPACITY only"
        self.capacity = capacity
        key = (str(device), capacity)
        if key not in _PRISTINE:                   # the fill is computed once per device and size; every arena gets a copy
            _PRISTINE[key] = torch.from_numpy(pattern(capacity).copy()).to(device)
        self.data = _PRISTINE[key].clone()
        self.expect = _PRISTINE[key].clone()
        self.free = torch.zeros(capacity, dtype=torch.bool, device=device)    # bytes a kernel may write
        self.base = self.data.data_ptr()
        self.windows = {}
        self.cursor = 0       # end of the last window
        self.guard = 0        # end of the last window's after-flank: no later window starts before it

    def sync(self):
        if self.data.is_cuda:
            torch.cuda.synchronize(self.data.device)

    def window(self, name, nbytes, align=16, phase=0, rows=1, pitch_bytes=None, kind="out") -> Window:
        """Reserve rows x nbytes bytes whose first byte sits `phase` bytes past an `align` boundary (of the address, not of
        the arena), a flank of max(64 KiB, the window's span) before and after it inside the allocation.  Between two windows
        lies the longer of the first one's after-flank and the second one's before-flank."""
        assert kind in KINDS and name not in self.windows and rows >= 1 and nbytes >= 0 and align >= 1
        pitch = nbytes if pitch_bytes is None else pitch_bytes
        assert pitch >= nbytes or rows == 1
        span = (rows - 1) * pitch + nbytes
        flank = max(MIN_FLANK, span)
        start = max(self.cursor + flank, self.guard)
        start += (phase - (self.base + start)) % align
        if start + span + flank > self.capacity:
            raise MemoryError(f"arena of {self.capacity} bytes is full at window {name!r} ({span} bytes + 2 flanks of {flank})")
        w = Window(self, name, kind, start, nbytes, rows, pitch)
        assert (w.ptr - phase) % align == 0
        self.cursor = start + span
        self.guard = self.cursor + flank
        self.windows[name] = w
        if kind != "in":
            torch.as_strided(self.free, (rows, nbytes), (pitch, 1), start).fill_(True)
        return w

    def _nearest(self, p):
        best = None
        for w in self.windows.values():
            side, off, row = w.locate(p)
            d = 0 if side in ("inside", "gap") else abs(off)
            if best is None or d < best[0]:
                best = (d, w, side, off, row)
        return best[1:] if best else (None, "unused", p, 0)

    def strays(self, limit=65536):
        """(total differing bytes, [per (window, side, row) dict]) -- the comparison runs on the device"""
        self.sync()
        bad = (self.data != self.expect) & ~self.free
        count = int(bad.sum().item())
        if not count:
            return 0, []
        pos = torch.nonzero(bad).reshape(-1)[:limit].cpu().numpy().tolist()
        groups = {}
        for p in pos:
            w, side, off, row = self._nearest(p)
            key = (w.name if w else None, side, row if side in ("gap", "inside") else 0)
            g = groups.get(key)
            if g is None:
                groups[key] = {"window": key[0], "side": side, "row": row, "offset": off, "far": off, "count": 1, "at": p,
                               "kind": w.kind if w else None}
            else:
                g["count"] += 1
                if abs(off) < abs(g["offset"]):
                    g["offset"], g["at"] = off, p
                if abs(off) > abs(g["far"]):
                    g["far"] = off
        return count, list(groups.values())

    def check(self):
        """Synchronise, then assert that nothing outside the out / inout windows changed.  The message names, for each window
        that was hit, the side (before / after / in a row gap / inside an `in` window), the signed byte offset of the nearest
        and the farthest stray byte from that edge (-1: the byte just before the window, +1: the byte just after it or after
        row r in a gap), and how many bytes differ."""
        count, groups = self.strays()
        if not count:
            return
        lines = [f"{count} byte(s) outside the output windows changed:"]
        for g in groups:
            w = self.windows.get(g["window"])
            where = {"before": "before", "after": "after", "gap": f"in the gap after row {g['row']} of",
                     "inside": f"inside row {g['row']} of", "unused": "in unused space near"}[g["side"]]
            shape = f" ({w.kind}, {w.rows} x {w.nbytes} bytes, pitch {w.pitch}, address % 128 = {w.ptr % 128})" if w else ""
            lines.append(f"  {g['count']} byte(s) {where} window {g['window']!r}{shape}: offsets {g['offset']:+d} .. {g['far']:+d} "
                         f"from that edge (arena byte {g['at']})")
        raise RedZoneError("\n".join(lines), groups, count)
