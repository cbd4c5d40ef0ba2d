"""Inflaters for the reader's device mode (``textio.TextReader``, ``CUTSEQ_GPU_INFLATE=1``): BGZF blocks go from the
mapped file straight into a text buffer.  The reader has one cutting loop (``textio._Pending``: k-th newline, carry,
growth) and two memories it runs in: the pinned arena (``textio._HostMemory``, which has ``take`` / ``give`` / ``copy`` /
``after_kth_newline`` below and nothing else) and an inflater, the memory of the BGZF source.  When that source ends,
``to_host`` brings what is left to the pinned arena, where the end of the input is decided.

Two of them with the same methods: :class:`DeviceInflater` wraps ``cs_inflate_*`` (the buffers are device memory, the
decoder is ``csrc/inflate_kernels.hip.inc``); :class:`HostInflater` does the same over numpy arrays with zlib, for the
CPU tests of the reader's loop.  Imported only when the switch is on.

  take(nbytes) -> buffer (``.size``; reused ones come from a pool)     give(buffer)
  inflate(mapped, lo, rows, buffer, at) -> (newlines per block, index of the first refused block or -1)
        rows: codec.bgzf_index's; the blocks' texts land back to back from buffer[at] on
  after_kth_newline(buffer, at, nbytes, k) -> offset behind newline k of buffer[at : at + nbytes], -1 without one
  copy(dst, dst_at, src, src_at, nbytes)        buffer to buffer
  to_host(array, src, src_at, nbytes)           buffer to a numpy array
  address(buffer)                               device address (DeviceInflater; what cs_text_submit_device takes)
"""
from __future__ import annotations

import ctypes as C
import threading
import zlib

import numpy as np

from . import abi

SPAN = 4 << 20          # compressed bytes per call, about
MAX_COMP = SPAN + (1 << 17)   # ... and the block that crosses the mark
MAX_BLOCKS = MAX_COMP // 28   # (the smallest BGZF block, the EOF marker, is 28 bytes)


class DeviceBuffer:
    __slots__ = ("addr", "size")

    def __init__(self, addr: int, size: int):
        self.addr, self.size = addr, size


class DeviceInflater:
    device_memory = True

    def __init__(self, device: int):
        from . import capi
        self.capi, self.L, self.device = capi, capi.load(), device
        self._h = C.c_void_p()
        capi.check(self.L.cs_inflate_create(device, MAX_COMP, MAX_BLOCKS, C.byref(self._h)))
        self._free, self._lock, self._closed = [], threading.Lock(), False
        self._live = 0

    def take(self, nbytes: int) -> DeviceBuffer:
        with self._lock:
            fit = [b for b in self._free if b.size >= nbytes]
            if fit:
                best = min(fit, key=lambda b: b.size)
                self._free.remove(best)
                self._live += 1
                return best
        addr = self.L.cs_alloc_device(self.device, max(nbytes, 1))
        if not addr:
            self.capi.check(abi.CS_ERR_NOMEM)
        with self._lock:
            self._live += 1
        return DeviceBuffer(addr, max(nbytes, 1))

    def give(self, buf: DeviceBuffer) -> None:
        with self._lock:
            self._live -= 1
            if not self._closed and len(self._free) < 12:
                self._free.append(buf)
                return
            last = self._closed and self._live == 0
        self.L.cs_free_device(self.device, buf.addr)
        if last:
            self._destroy()

    def address(self, buf: DeviceBuffer) -> int:
        return buf.addr

    def inflate(self, mapped, lo: int, rows, buf: DeviceBuffer, at: int):
        n = len(rows)
        table = np.zeros(n, dtype=abi.INFLATE_BLOCK_DTYPE)
        r = np.asarray(rows, dtype=np.int64).reshape(n, 4)
        table["comp_off"] = r[:, 0] - lo
        table["comp_len"] = r[:, 1]
        table["out_len"] = r[:, 2]
        table["crc32"] = r[:, 3]
        table["out_off"] = at + np.concatenate(([0], np.cumsum(r[:, 2])[:-1]))
        hi = int(r[-1, 0] + r[-1, 1])
        base = mapped.ctypes.data  # (a uint8 array over the mapped file)
        lines = np.zeros(n, dtype=np.uint32)
        res = abi.cs_inflate_result()
        self.capi.check(self.L.cs_inflate_bgzf(self._h, base + lo, hi - lo, table.ctypes.data, n, buf.addr, buf.size,
                                               lines.ctypes.data, None, C.byref(res)))
        return lines, (int(res.block) if res.verdict != abi.CS_INFLATE_OK else -1)

    def after_kth_newline(self, buf: DeviceBuffer, at: int, nbytes: int, k: int) -> int:
        got = C.c_int64(-1)
        self.capi.check(self.L.cs_dtext_after_kth_newline(self.device, buf.addr + at, nbytes, k, C.byref(got)))
        return int(got.value)

    def copy(self, dst: DeviceBuffer, dst_at: int, src: DeviceBuffer, src_at: int, nbytes: int) -> None:
        if nbytes:
            self.capi.check(self.L.cs_copy_on_device(self.device, dst.addr + dst_at, src.addr + src_at, nbytes))

    def to_host(self, arr: np.ndarray, src: DeviceBuffer, src_at: int, nbytes: int) -> None:
        if nbytes:
            self.capi.check(self.L.cs_copy_to_host(self.device, arr.ctypes.data, src.addr + src_at, nbytes))

    def _destroy(self):
        if self._h:
            self.L.cs_inflate_destroy(self._h)
            self._h = C.c_void_p()

    def close(self) -> None:
        """The pool's buffers go now; buffers still out (blocks on their way through a worker) when they come back."""
        with self._lock:
            self._closed = True
            free, self._free = self._free, []
            last = self._live == 0
        for b in free:
            self.L.cs_free_device(self.device, b.addr)
        if last:
            self._destroy()


class HostInflater:
    """The same over numpy arrays and zlib: what the CPU tests run the reader's device mode on."""
    device_memory = False

    def take(self, nbytes: int) -> np.ndarray:
        return np.empty(max(nbytes, 1), dtype=np.uint8)

    def give(self, buf) -> None:
        pass

    def address(self, buf) -> int:
        return buf.ctypes.data

    def inflate(self, mapped, lo: int, rows, buf, at: int):
        lines = np.zeros(len(rows), dtype=np.uint32)
        for i, (start, nbytes, isize, crc) in enumerate(rows):
            d = zlib.decompressobj(-15)
            try:
                text = d.decompress(bytes(mapped[start:start + nbytes]))
            except zlib.error:
                return lines, i
            if not d.eof or d.unused_data or len(text) != isize or zlib.crc32(text) != crc:
                return lines, i
            buf[at:at + isize] = np.frombuffer(text, dtype=np.uint8)
            lines[i] = text.count(b"\n")
            at += isize
        return lines, -1

    def after_kth_newline(self, buf, at: int, nbytes: int, k: int) -> int:
        if k < 1:
            return 0
        ends = np.flatnonzero(buf[at:at + nbytes] == 10)
        return int(ends[k - 1]) + 1 if k <= ends.size else -1

    def copy(self, dst, dst_at: int, src, src_at: int, nbytes: int) -> None:
        dst[dst_at:dst_at + nbytes] = src[src_at:src_at + nbytes]

    def to_host(self, arr, src, src_at: int, nbytes: int) -> None:
        arr[:nbytes] = src[src_at:src_at + nbytes]

    def close(self) -> None:
        pass
