"""Host side of the text path: blocks of whole FASTQ records in, output streams out.

What is left for the host once the device parses and formats (``cs_text_*``, ``textpath.py``): read (or inflate)
the input, cut it into blocks of exactly ``chunk_reads`` records -- two vectorised passes over the bytes, newline
count and k-th newline, no per-record work -- and write (or deflate) the finished output text, strictly in input
order.  Counterpart of ``runner.run(pipeline, Progress(), outfiles)`` with ``make_runner(cores=N)``
(cutseq/run.py:436, 473, 753, 794): reader, chunk fan-out to workers, ordered merge.

  TextReader    one thread per input file and one cutting loop with two memories: a source (page cache, several
                ``pread`` calls at once; the inflate pool; BGZF spans through an inflater, CUTSEQ_GPU_INFLATE) appends
                to ``_Pending``, which cuts behind newline 4 * chunk_reads and carries the rest -- in pinned memory or
                in the inflater's (device memory) -> ``TextBlock(buf, nbytes, n_records)``.  An unaligned BAM input
                (by content) is the same loop with a second unit: ``_PendingRecords`` cuts in front of record
                chunk_reads of the length-prefixed chain (``csh_bam_walk``); its blocks hold raw records, their offsets
                and the size of the text the device expands them to (``cs_text_submit_bam``)
  TextWorker    one thread per GPU (a ``fanout.Worker``): a ``TrimEngine`` + ``TextEngine``, three batches in flight;
                grows the row stride or the text capacity when a batch needs it
  run_text_pipeline   pairs the mates' blocks and hands them to ``fanout.run_ordered`` (round-robin deal, results back
                in input order), which feeds one ``StreamWriter`` per output file (plain: parallel ``pwrite``;
                ``.gz``: 4 MB gzip members from the pool)

Every run takes this path by default, demultiplexing runs included (``--demux-barcodes``: routes 3 + b).  The record
path (``run.run_pipeline`` with the native parser / formatter of ``cutseq_host.c``) is a second host implementation
behind ``CUTSEQ_TEXT_PATH=0``, held to the same outputs by the tests' switch matrix.
"""
from __future__ import annotations

import concurrent.futures
import ctypes as C
import dataclasses
import mmap
import os
import queue
import threading
import time
from typing import List, Optional

import numpy as np

from . import abi, codec, fanout, fastq, rename, report, switches, textpath
from .abi import ReadTooLong
from .outputs import TextOptions

CHUNK_READS = 1 << 18
_BLOCK = 8 << 20          # bytes per pread / per inflate hand-over
_GZ_PIECE = 4 << 20       # output text per gzip member
_COPY_PIECE = 4 << 20     # plain output: bytes per parallel copy into the file mapping
_MAP_MIN = 8 << 20        # ... used from this size on (smaller pieces go through pwrite)
_PAGE = mmap.ALLOCATIONGRANULARITY


PROFILE = switches.enabled("PROFILE")  # (sampled once, when the module is imported)
_DISCARD = False
_prof = {}
_prof_lock = threading.Lock()


def _tick(key: str, t0: float) -> float:
    """Diagnostic (CUTSEQ_PROFILE=1): seconds per thread and activity, printed at the end of the run."""
    now = time.perf_counter()
    if PROFILE:
        name = f"{threading.current_thread().name}:{key}"
        with _prof_lock:
            _prof[name] = _prof.get(name, 0.0) + (now - t0)
    return now


_inflate_blocks = {"device_blocks": 0, "host_blocks": 0}  # (CUTSEQ_PROFILE=1: who inflated the gzip inputs' blocks)


def _count_inflate(key: str, n: int) -> None:
    with _prof_lock:
        _inflate_blocks[key] += n


def _host():
    L = fastq._lib()
    if not getattr(L, "_text_bound", False):
        L.csh_count_newlines.restype = C.c_int64
        L.csh_count_newlines.argtypes = [C.c_void_p, C.c_int64]
        L.csh_after_kth_newline.restype = C.c_int64
        L.csh_after_kth_newline.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
        L.csh_fasta_to_fastq.restype = C.c_int64
        L.csh_fasta_to_fastq.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.csh_bam_header.restype = C.c_int64
        L.csh_bam_header.argtypes = [C.c_void_p, C.c_int64]
        L.csh_bam_walk.restype = C.c_int64
        L.csh_bam_walk.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        L._text_bound = True
    return L


class TextBlock:
    """``n_records`` complete records in ``buf[:nbytes]`` (a pinned arena buffer) -- or, from a reader in device mode,
    in the first ``nbytes`` of ``dbuf``, a buffer of the inflater ``owner`` (``buf`` is None then).  A block of a BAM
    input holds raw BAM records: ``offsets`` (a pinned buffer read as uint32) has their starts and the end of the last
    one, ``text_bytes`` is the size of the FASTQ text they expand to."""

    __slots__ = ("buf", "nbytes", "n", "first_record", "dbuf", "owner", "offsets", "text_bytes")

    def __init__(self, buf: Optional[np.ndarray], nbytes: int, n: int, first_record: int, dbuf=None, owner=None,
                 offsets: Optional[np.ndarray] = None, text_bytes: int = 0):
        self.buf, self.nbytes, self.n, self.first_record = buf, nbytes, n, first_record
        self.dbuf, self.owner = dbuf, owner
        self.offsets, self.text_bytes = offsets, text_bytes

    def text_size(self) -> int:
        """Bytes of the text the block is (or becomes on the device): what sizes the slot."""
        return self.text_bytes if self.offsets is not None else self.nbytes

    def text_address(self) -> int:
        """Where the text is: a host address, or a device address (``dbuf``)."""
        return self.owner.address(self.dbuf) if self.dbuf is not None else self.buf.ctypes.data

    def release(self) -> None:
        if self.buf is not None:
            fastq.PINNED.give(self.buf)
            self.buf = None
        if self.offsets is not None:
            fastq.PINNED.give(self.offsets)
            self.offsets = None
        if self.dbuf is not None:
            self.owner.give(self.dbuf)
            self.dbuf = None


class _HostMemory:
    """The pinned arena under the inflater's method names (``inflater.py``): the memory the reader cuts host text in."""

    def take(self, nbytes: int) -> np.ndarray:
        return fastq.PINNED.take(nbytes)

    def give(self, buf: np.ndarray) -> None:
        fastq.PINNED.give(buf)

    def copy(self, dst: np.ndarray, dst_at: int, src: np.ndarray, src_at: int, nbytes: int) -> None:
        C.memmove(dst.ctypes.data + dst_at, src.ctypes.data + src_at, nbytes)

    def after_kth_newline(self, buf: np.ndarray, at: int, nbytes: int, k: int) -> int:
        return int(_host().csh_after_kth_newline(buf.ctypes.data + at, nbytes, k))


_HOST = _HostMemory()


class _Pending:
    """The text behind the last block that went out: ``buf[:fill]``, a buffer of ``mem`` (:class:`_HostMemory` or an
    inflater), holds ``lines`` newlines; ``marks`` has one (offset, nbytes, newlines) per piece a source appended.
    ``goal`` (the lines the loop is filling up to) and ``est`` are there for the sources to size their reads by.
    The unit the loop counts and cuts by is the line, ``per_record`` of them to a record; :class:`_PendingRecords`
    counts whole BAM records instead."""

    per_record = 4

    def __init__(self, mem, chunk_reads: int):
        self.mem, self.chunk_reads = mem, chunk_reads
        self.est = 400  # bytes per record, corrected by every block that goes out
        self.buf = mem.take(self.size())
        self.fill = self.lines = self.goal = 0
        self.marks: List[tuple] = []
        self.copies: List = []  # pieces on their way into `buf` (copied by the pool)

    def size(self) -> int:
        return int(self.chunk_reads * self.est * 1.25) + 2 * _BLOCK

    def settle(self) -> None:
        """Pooled copies into ``buf`` are awaited before it is read, grown, cut, moved or given back: here, all of them."""
        copies, self.copies = self.copies, []
        for f in concurrent.futures.wait(copies).done:
            f.result()

    def room(self, nbytes: int) -> None:
        """``nbytes`` free bytes behind ``fill``, in a bigger buffer if need be."""
        if self.buf.size - self.fill < nbytes:
            self.settle()
            bigger = self.mem.take(max(self.buf.size + self.buf.size // 2, self.fill + nbytes))
            self.mem.copy(bigger, 0, self.buf, 0, self.fill)
            self.mem.give(self.buf)
            self.buf = bigger

    def added(self, nbytes: int, newlines: int) -> None:
        self.marks.append((self.fill, nbytes, newlines))
        self.fill += nbytes
        self.lines += newlines

    def refresh(self) -> None:
        """The units in ``buf[:fill]`` are counted, up to ``goal`` (lines are, piece by piece, as they arrive)."""

    def _cut_point(self, k: int):
        """-> (the offset behind unit ``k``, what a block of this unit needs beyond its bytes -- lines: nothing); what
        the pending keeps about its pieces is moved up to the cut.  ``marks`` say which piece holds the newline, and only
        that piece is searched for it."""
        cum = 0
        for at, (off, nbytes, found) in enumerate(self.marks):
            if cum + found >= k:
                break
            cum += found
        cut = off + self.mem.after_kth_newline(self.buf, off, nbytes, k - cum)
        assert cum + found >= k and cut > 0
        # the piece the cut went through keeps its rest, the others move up
        self.marks = [(0, off + nbytes - cut, found - (k - cum))] + [(o - cut, n, f) for o, n, f in self.marks[at + 1:]]
        return cut, None

    def cut(self, k: int):
        """-> (buffer, cut, extra): the text up to unit ``k`` (newline ``k``) leaves in its buffer, what is behind it is
        carried into a fresh one.  ``extra``: :meth:`_cut_point`'s."""
        cut, extra = self._cut_point(k)
        nxt = self.mem.take(max(self.buf.size, self.size()))
        self.mem.copy(nxt, 0, self.buf, cut, self.fill - cut)
        old, self.buf = self.buf, nxt
        self.fill, self.lines = self.fill - cut, self.lines - k
        return old, cut, extra

    def end_of_input(self, path: str):
        """What is left when the source has ended -> ``_end_of_input``'s triple and the last block's ``extra``."""
        return _end_of_input(memoryview(self.buf)[:self.fill], path) + (None,)

    def drop_lines(self, k: int) -> None:
        self.mem.give(self.cut(k)[0])

    def to_host(self, spare: int) -> None:
        """From an inflater's buffer into a pinned one with ``spare`` bytes of room (the pieces stay where they are)."""
        buf = _HOST.take(self.fill + spare)
        self.mem.to_host(buf, self.buf, 0, self.fill)
        self.mem.give(self.buf)
        self.mem, self.buf = _HOST, buf

    def close(self) -> None:
        try:
            self.settle()
        except BaseException:
            pass
        if self.buf is not None:
            self.mem.give(self.buf)
            self.buf = None


class _PendingRecords(_Pending):
    """:class:`_Pending` for an unaligned BAM input: the unit is the whole record (``per_record`` 1), ``lines`` counts
    the records found behind the header.  Records are length-prefixed, so their starts are a serial chain:
    ``csh_bam_walk`` follows it over what has arrived (:meth:`refresh`), never further than the loop's ``goal``, and notes
    every start; a cut is the noted start of record ``k``.  Pieces need no marks."""

    per_record = 1

    def __init__(self, mem, chunk_reads: int, path: str):
        super().__init__(mem, chunk_reads)
        self.path = path
        self.header = False   # the BAM header has been dropped from the front
        self.records_out = 0  # records in the blocks that left (for messages)
        self.walked = 0       # buf[:walked] is `lines` whole records
        self.text = 0         # ... that expand to this much FASTQ text
        self.offs = fastq.PINNED.take(4 * (chunk_reads + 1))

    def added(self, nbytes: int, newlines: int) -> None:
        self.fill += nbytes

    def _skip_header(self) -> bool:
        size = int(_host().csh_bam_header(self.buf.ctypes.data, self.fill))
        if size == -1:
            raise fastq.FastqFormatError(f"{self.path}: malformed BAM: the stream does not start with the magic 'BAM\\1'")
        if size == -2:
            raise fastq.FastqFormatError(f"{self.path}: malformed BAM: a negative length in the header")
        if size == 0:
            return False
        self.mem.copy(self.buf, 0, self.buf, size, self.fill - size)  # (memmove: the ranges overlap)
        self.fill -= size
        self.header = True
        return True

    def refresh(self) -> None:
        want = self.goal - self.lines
        if want <= 0:
            return
        self.settle()  # (the chain is followed over bytes that have arrived)
        if not self.header and not self._skip_header():
            return
        if self.fill >= 1 << 31:
            raise ReadTooLong(f"{self.path}: a block of BAM records outgrew 2 GiB (smaller blocks: CUTSEQ_CHUNK_READS)", 0)
        offs = self.offs.view(np.uint32)
        nxt, text, bad = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        t0 = time.perf_counter()
        found = int(_host().csh_bam_walk(self.buf.ctypes.data, self.fill, self.walked, want, offs[self.lines:].ctypes.data,
                                         C.byref(nxt), C.byref(text), C.byref(bad)))
        _tick("bam_walk", t0)
        self.lines += found
        self.walked, self.text = int(nxt.value), self.text + int(text.value)
        if bad.value:
            raise fastq.FastqFormatError(
                f"{self.path}: malformed BAM: record {self.records_out + self.lines} has a block_size below 32")

    def _block_extra(self, k: int):
        """The offsets of the first ``k`` records and the end of the last one, in a buffer of their own."""
        assert k == self.lines, "the walk stops at the goal: a cut takes every record found"
        out = fastq.PINNED.take(4 * (k + 1))
        offs = out.view(np.uint32)
        offs[:k] = self.offs.view(np.uint32)[:k]
        offs[k] = self.walked
        return out, self.text

    def _cut_point(self, k: int):
        extra = self._block_extra(k)
        cut, self.walked, self.text = self.walked, 0, 0
        self.records_out += k
        return cut, extra

    def end_of_input(self, path: str):
        if not self.header:
            raise fastq.FastqFormatError(f"{path}: malformed BAM: the stream ends inside the header")
        if self.walked < self.fill:
            raise fastq.FastqFormatError(
                f"{path}: malformed BAM: the stream ends inside record {self.records_out + self.lines}")
        return self.fill, self.lines, False, (self._block_extra(self.lines) if self.lines else None)

    def close(self) -> None:
        super().close()
        if self.offs is not None:
            fastq.PINNED.give(self.offs)
            self.offs = None


def _copy_in(dst: int, text: np.ndarray, nbytes: int) -> None:
    C.memmove(dst, text.ctypes.data, nbytes)
    if isinstance(text.base, fastq.mmap.mmap):
        fastq.ARENA.give(text)


def _end_of_input(text, path: str):
    """``text``: what is left at the end of the input -> (end, records, append_newline): ``text[:end]`` is the last
    block's ``records`` whole records, after a '\\n' is written at ``text[end - 1]`` if ``append_newline`` says so.

    What is left must be whole records; blank lines behind the last one are tolerated.  The last NON-BLANK line
    decides: it is line 4k + 3 (a quality line: the record ends with it, the device takes the end of the text for its
    missing line end) or line 4k + 2 (a '+' line: the record has an empty read, "@id\\n\\n+\\n\\n", and its empty quality
    line is the first blank line behind it).  Only whole blank lines beyond that are dropped -- stripping all trailing
    white space took the empty quality line with it and turned a valid file into "truncated"."""
    view = memoryview(text)
    fill = end = len(view)
    while end > 0 and view[end - 1] in b"\n\r \t":
        end -= 1
    if end == 0:
        return 0, 0, False
    last = int(_host().csh_count_newlines(np.frombuffer(view, dtype=np.uint8).ctypes.data, end))  # index of the last non-blank line
    if last % 4 == 3:
        return end, (last + 1) // 4, False
    if last % 4 == 2 and end < fill:
        # the '+' line's own line end, then the empty quality line (its '\n' is written if the file lacks it)
        tail = bytes(view[end:fill])  # white space only
        nl1 = tail.find(b"\n")
        if nl1 >= 0:
            nl2 = tail.find(b"\n", nl1 + 1)
            return (end + nl2 + 1 if nl2 >= 0 else fill + 1), (last + 2) // 4, nl2 < 0
    raise fastq.FastqFormatError(f"{path}: truncated FASTQ record at end of file")


class TextReader(threading.Thread):
    """One input file -> :class:`TextBlock` objects of exactly ``chunk_reads`` records (the last one may be shorter),
    then ``None``.  Exceptions travel through the queue."""

    def __init__(self, path: str, chunk_reads: int, start: int = 0, skip_lines: int = 0, max_records: Optional[int] = None,
                 stop: Optional[int] = None, interleaved: bool = False, inflater=None):
        """``interleaved``: the file holds pairs, mate 1 and mate 2 alternating (``--interleaved``).  ``chunk_reads`` still
        counts records and must be even, so every block holds whole pairs; a block's ``n`` and ``first_record`` count
        pairs.  A file that ends on an odd record is refused (:meth:`pair_count`).
        ``start`` / ``skip_lines`` / ``max_records`` / ``stop``: one rank's share of the file in the multi-process form
        (``ranks.py``): begin at byte ``start`` (plain text) or at the gzip member that starts there, drop
        ``skip_lines`` lines, stop behind ``max_records`` records (None = to the end of the file) or in front of the
        gzip member that starts at compressed offset ``stop``.
        ``inflater``: a callable that makes an inflater (``inflater.py``) -- the device mode, for a whole gzip FASTQ file
        that starts with a BGZF block: the blocks are inflated into the inflater's buffers (device memory), the blocks
        handed out hold such a buffer, and only what is left when the BGZF run ends comes back to the host path.  Any
        other input ignores it (the callable is not called)."""
        super().__init__(daemon=True, name=f"cutseq-read-{os.path.basename(path)}")
        self.path, self.chunk_reads = path, chunk_reads
        self.start_at, self.skip_lines, self.max_records, self.stop_at = start, skip_lines, max_records, stop
        self.interleaved = interleaved
        if interleaved and (chunk_reads % 2 or start or skip_lines or max_records is not None or stop is not None):
            raise ValueError(f"{path}: an interleaved input is read whole, in blocks of an even number of records")
        self.blocks: "queue.Queue" = queue.Queue(maxsize=3)
        self._halt = False
        # What the file holds decides how it is read (dnaio / xopen go by content too, cutseq/run.py:434-441, 751-758):
        # gzip and plain FASTQ files take the parallel paths; standard input ("-"), bzip2 / xz / zstandard files and
        # FASTA text come through a sequential reader (codec.StreamSource), FASTA re-shaped into four-line records.
        self.container, first, self._opener = codec.sniff_input(path)
        self.fasta = first[:1] in (b">", b"#")  # (dnaio: a leading comment line means FASTA too)
        # an unaligned BAM (a BGZF container whose text starts "BAM\1"): the same sources, records cut by their lengths
        self.bam = codec.is_bam(self.container, first)
        self.sequential = path == "-" or self.container in ("bz2", "xz", "zst") or (self.fasta and self.container == "plain")
        self.gz = self.container == "gzip" and not self.sequential
        if (self.sequential or self.fasta or self.bam or (stop is not None and not self.gz)) and (
                start or skip_lines or max_records is not None or stop is not None):
            raise ValueError(f"{path}: only plain and gzip FASTQ files can be split between ranks")
        self._make_inflater = None
        if (inflater is not None and self.gz and not self.fasta and not self.bam and not interleaved and codec.libdeflate() is not None
                and not (start or skip_lines or max_records is not None or stop is not None)):
            with open(path, "rb") as fh:
                if codec._bgzf_block_size(fh.read(1 << 16), 0):
                    self._make_inflater = inflater
        self.start()

    # -- plumbing ---------------------------------------------------------------------------------------
    def _put(self, item) -> bool:
        t0 = time.perf_counter()
        try:
            while not self._halt:
                try:
                    self.blocks.put(item, timeout=0.2)
                    return True
                except queue.Full:
                    continue
            return False
        finally:
            _tick("blocked_on_consumer", t0)

    def get(self) -> Optional[TextBlock]:
        item = self.blocks.get()
        if isinstance(item, fastq._Failure):
            raise item.exc
        return item

    def close(self) -> None:
        self._halt = True
        deadline = time.monotonic() + 30.0
        while self.is_alive() and time.monotonic() < deadline:
            try:
                while True:
                    item = self.blocks.get_nowait()
                    if isinstance(item, TextBlock):
                        item.release()
            except queue.Empty:
                pass
            self.join(timeout=0.05)

    @staticmethod
    def pair_count(records: int, path: str) -> int:
        """Pairs in a block of ``records`` records of an interleaved input; only the last block can be odd."""
        if records % 2:
            raise fastq.FastqFormatError(
                f"{path}: the interleaved input is incomplete: it ends after an odd number of records, the last record "
                "has no partner.")
        return records // 2

    def _block(self, mem, buf, nbytes: int, records: int, done: int, extra=None) -> TextBlock:
        """The block of ``records`` records behind the ``done`` records handed out so far, in a buffer of ``mem``.
        ``extra``: a BAM block's (offsets, text bytes)."""
        if mem is not _HOST:
            return TextBlock(None, nbytes, records, done, dbuf=buf, owner=mem)
        offsets, text_bytes = extra if extra is not None else (None, 0)
        if self.interleaved:
            try:
                return TextBlock(buf, nbytes, self.pair_count(records, self.path), done // 2, offsets=offsets, text_bytes=text_bytes)
            except BaseException:
                if offsets is not None:
                    fastq.PINNED.give(offsets)
                raise
        return TextBlock(buf, nbytes, records, done, offsets=offsets, text_bytes=text_bytes)

    @staticmethod
    def _members_until(src, start: int, stop: int):
        """The blocks of the members in [start, stop) (compressed offsets; the share of a rank that splits by members)."""
        gen = src.indexed_blocks(start)
        try:
            for off, arr, nbytes in gen:
                if off >= stop:
                    src.give(arr)
                    return
                yield arr, nbytes
        finally:
            gen.close()

    @staticmethod
    def _fasta_convert(data: bytes, out: np.ndarray, final: bool):
        """-> (bytes written | -1 | -2, bytes of ``data`` consumed, line of a format error)"""
        consumed, records, err_line = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        produced = _host().csh_fasta_to_fastq(data, len(data), out.ctypes.data, out.size, 1 if final else 0, 0,
                                              C.byref(consumed), C.byref(records), C.byref(err_line))
        return int(produced), int(consumed.value), int(err_line.value)

    # -- sources: generators that append text to a _Pending, one round per step, and end with their input ------------
    def _plain_text(self, pend: _Pending, pos: int):
        """The plain file from byte ``pos`` on: several preads (and newline counts) at once in the pool."""
        L = _host()
        fd = os.open(self.path, os.O_RDONLY)
        try:
            eof = False
            while not eof:
                t0 = time.perf_counter()
                want = max(_BLOCK, int((pend.goal - pend.lines) / 4 * pend.est * 1.05))
                pieces = max(1, min(16, (want + _BLOCK - 1) // _BLOCK))  # (a block of 262 144 short-read records: 11 pieces, one round)
                pend.room(pieces * _BLOCK)
                fill, base, mv = pend.fill, pend.buf.ctypes.data, memoryview(pend.buf)

                def job(i):
                    off = fill + i * _BLOCK
                    got = 0
                    while got < _BLOCK:  # a short read is not the end of the file (FUSE, network mounts): only 0 bytes is
                        more = os.preadv(fd, [mv[off + got:off + _BLOCK]], pos + i * _BLOCK + got)
                        if more <= 0:
                            break
                        got += more
                    return got, (int(L.csh_count_newlines(base + off, got)) if got else 0)

                pool = fastq._pool()
                results = [f.result() for f in [pool.submit(job, i) for i in range(pieces)]] if pieces > 1 else [job(0)]
                for got, lines in results:
                    if eof and got:  # a short piece in the middle: the file changed under us
                        raise OSError(f"{self.path}: short read")
                    if got:
                        pend.added(got, lines)
                    eof = got < _BLOCK
                pos += pend.fill - fill
                _tick("read", t0)
                yield True
        finally:
            os.close(fd)

    def _block_text(self, pend: _Pending, pos: int):
        """Blocks of text from a generator -- gzip members from compressed offset ``pos`` on, inflated in the pool, or a
        sequential stream, FASTA re-shaped into four-line records --, copied in by the pool."""
        L = _host()
        if self.gz and not self.fasta:
            # (a BAM's blocks hold no lines to count: its records are found once the bytes stand in a row)
            count = None if self.bam else (lambda addr, nbytes: int(L.csh_count_newlines(addr, nbytes)))
            src = codec.GzipSource(self.path, fastq._pool(), fastq.ARENA.take, fastq.ARENA.give, post=count)
            gen = src.blocks(pos) if self.stop_at is None else self._members_until(src, pos, self.stop_at)
            if pos >= src.size:  # (a BGZF run that went through the inflater was the whole file)
                gen = iter(())
        else:
            if self.gz:  # (FASTA in a gzip file: the members still inflate in the pool)
                src = codec.GzipSource(self.path, fastq._pool(), fastq.ARENA.take, fastq.ARENA.give)
            else:
                src = codec.StreamSource(self._opener(), fastq.ARENA.take, fastq.ARENA.give)
            if self.fasta:
                src = codec.FastaSource(src, self._fasta_convert, fastq.ARENA.take, fastq.ARENA.give, self.path)
            gen = src.blocks(0)
        try:
            for text, nbytes in gen:
                if self.gz and PROFILE:
                    _count_inflate("host_blocks", 1)
                pend.room(nbytes)
                got = src.side(text)
                if self.bam:
                    got = 0
                elif got is None:
                    got = int(L.csh_count_newlines(text.ctypes.data, nbytes))
                pend.copies.append(fastq._pool().submit(_copy_in, pend.buf.ctypes.data + pend.fill, text, nbytes))
                pend.added(nbytes, got)
                yield True
        finally:
            if hasattr(gen, "close"):
                gen.close()
            src.close()

    def _host_text(self, pend: _Pending, pos: int):
        return self._block_text(pend, pos) if self.gz or self.sequential else self._plain_text(pend, pos)

    def _refused(self, mapped, lo: int, hi: int, index: int):
        """The inflater refused block ``index`` of the span [lo, hi): the host path decides.  What it raises for a corrupt
        file today, it raises now; if it takes the span, the two decoders disagree, and that is an engine fault."""
        out, _used = codec._inflate_span(mapped, lo, hi, 4 * (hi - lo), fastq.ARENA.take, fastq.ARENA.give)
        fastq.ARENA.give(out)
        raise RuntimeError(f"{self.path}: the device decoder disagrees with libdeflate: it refused BGZF block {index} of "
                           f"the blocks at compressed offset {lo}, which libdeflate inflates without an error")

    def _bgzf_text(self, pend: _Pending):
        """The device mode: the BGZF blocks at the head of the file, a span at a time, inflated into ``pend``'s buffer by
        its memory, an inflater (``inflater.py``); one piece per block (ISIZE, newlines from the inflater).  When the run
        ends -- the end of the file, a member that is not BGZF, a block cut short -- what is left goes to a pinned host
        buffer and the host's source goes on behind it: a foreign tail member, blank lines, a missing final newline, an
        empty last read are all the host's business, in one place."""
        from .inflater import SPAN
        inf, pos = pend.mem, 0
        fh = open(self.path, "rb")
        mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
        mapped = np.frombuffer(mm, dtype=np.uint8)
        try:
            while True:
                rows, end = codec.bgzf_index(mm, pos, pos + SPAN + (1 << 16))
                if not rows:
                    break
                pend.room(sum(r[2] for r in rows))  # (known beforehand: the ISIZE prefix sums are the output offsets)
                t0 = time.perf_counter()
                got, bad = inf.inflate(mapped, pos, rows, pend.buf, pend.fill)
                _tick("device_inflate", t0)
                if bad >= 0:
                    self._refused(mm, pos, end, bad)
                for (_, _, isize, _), found in zip(rows, got):
                    pend.added(isize, int(found))
                if PROFILE:
                    _count_inflate("device_blocks", len(rows))
                pos = end
                yield True
            pend.to_host(2 * _BLOCK)
            inf.close()
        finally:
            del mapped
            try:
                mm.close()
            except BufferError:
                pass
            fh.close()
        yield from self._host_text(pend, pos)

    # -- the one cutting loop: fill up to `need` lines, cut, carry -- in pinned memory or in an inflater's ------------------
    def _cut_blocks(self, pend: _Pending, source) -> None:
        done, skip = 0, self.skip_lines
        left = self.max_records  # records still to hand out (None: everything)

        per = pend.per_record  # units (lines; whole records of a BAM input) to a record

        def fill(goal: int) -> None:
            pend.goal = goal
            pend.refresh()
            while pend.lines < goal and next(source, False):
                pend.refresh()
            pend.settle()

        while not self._halt and left != 0:
            need = per * (self.chunk_reads if left is None else min(self.chunk_reads, left))
            if skip:  # (the share starts `skip` lines into its first gzip member)
                fill(skip)
                if pend.lines >= skip:
                    pend.drop_lines(skip)
                    skip = 0
            fill(need)
            if pend.lines < need:  # the end of the input (a source that ends leaves the text in pinned memory)
                end, records, newline, extra = pend.end_of_input(self.path)
                if records and newline:
                    pend.room(1)
                    pend.buf[end - 1] = 0x0A
                if records:
                    block, pend.buf = self._block(_HOST, pend.buf, end, records, done, extra), None
                    if not self._put(block):
                        block.release()
                        return
                break
            # the block ends right behind newline number `need` (in front of BAM record number `need`)
            t0 = time.perf_counter()
            buf, cut, extra = pend.cut(need)
            block = self._block(pend.mem, buf, cut, need // per, done, extra)
            done += need // per
            if left is not None:
                left -= need // per
            pend.est = max(64, cut // (need // per) + 1)
            _tick("cut+carry", t0)
            if not self._put(block):
                block.release()
                return
        self._put(None)

    def run(self):
        try:
            mem = self._make_inflater() if self._make_inflater is not None else _HOST
            pend = _PendingRecords(mem, self.chunk_reads, self.path) if self.bam else _Pending(mem, self.chunk_reads)
            source = self._bgzf_text(pend) if mem is not _HOST else self._host_text(pend, self.start_at)
            try:
                self._cut_blocks(pend, source)
            finally:
                pend.close()
                source.close()
                if pend.mem is not _HOST:  # (the BGZF source closes the inflater behind its last block; it did not get there)
                    pend.mem.close()
        except BaseException as exc:
            self._put(fastq._Failure(exc))


class _Shared:
    """Output buffers of one batch on their way to several files: released when the last writer is done."""

    def __init__(self, bufs, consumers: int, on_release):
        self.bufs, self.left, self.on_release = bufs, consumers, on_release
        self.lock = threading.Lock()
        if consumers == 0:
            self._release()

    def _release(self):
        for b in self.bufs:
            fastq.PINNED.give(b)
        self.bufs = ()
        self.on_release()

    def done(self):
        with self.lock:
            self.left -= 1
            last = self.left == 0
        if last:
            self._release()


_libc = None


def _bind_libc():
    global _libc
    if _libc is None:
        try:
            _libc = C.CDLL(None, use_errno=True)
            _libc.fallocate.restype = C.c_int
            _libc.fallocate.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int64]
        except (OSError, AttributeError):
            _libc = False
    return _libc


def _fallocate(fd: int, offset: int, length: int) -> bool:
    """Linux fallocate(2), mode 0 (extends the file) -> False when the file system has no such thing.  (Not
    os.posix_fallocate: glibc emulates a missing fallocate by touching every block.)"""
    if not _bind_libc():
        return False
    if _libc.fallocate(fd, 0, offset, length) == 0:
        return True
    err = C.get_errno()
    import errno
    if err in (errno.EOPNOTSUPP, errno.ENOSYS, errno.EINVAL, errno.ENODEV, errno.ESPIPE):
        return False  # this file (system) cannot do it: the caller truncates instead
    raise OSError(err, os.strerror(err))  # disk full, file too large, ...: better here than as SIGBUS in a mapping


class StreamWriter:
    """One output file, written strictly in the order of :meth:`put`.  ``.gz``: the text goes out as gzip members
    of about 4 MB, compressed in the pool (level 1 = cutadapt's default; any split of the text is a valid gzip
    file and decompresses to the same bytes); plain: big pieces are written with several ``pwrite`` calls at once."""

    def __init__(self, path: str, level: int = 1, precompressed: bool = False, bgzf: bool = False):
        """``precompressed``: what arrives are finished gzip members (the device compressed them): written as they are.
        ``bgzf`` (``--bgzf``; a gzip file only): the file is BGZF -- the host branch compresses into blocks
        (``codec.bgzf_blocks``), the precompressed branch takes the device's blocks -- and :meth:`close` ends it with
        the EOF marker."""
        # xopen's rules (cutseq/run.py:437, 754: OutputFiles): the container goes by the name's extension, "-" is
        # standard output.  gzip and plain files keep their parallel paths; bzip2 / xz / zstandard streams are
        # compressed by this writer's own thread (stdlib codecs), standard output takes sequential writes.
        self.path, self.level = path, level
        self.container = codec.container_of_name(path) if path != "-" else "plain"
        self.gz = self.container == "gzip"
        self.precompressed = precompressed and self.gz
        self.bgzf = bgzf and self.gz
        self.codec = codec.make_compressor(self.container, level) if self.container in ("bz2", "xz", "zst") else None
        self.stdout = path == "-"
        if self.stdout:
            import sys
            sys.stdout.flush()
            self.fd = os.dup(1)
        else:
            self.fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o666)
        self.pos = 0
        # (gzip members are small: plain pwrite, the pool has better things to do)
        self.mappable = self.container == "plain" and not self.stdout
        self._can_allocate = True    # plain output: fallocate works on this file (system)
        self.q: "queue.Queue" = queue.Queue()
        self.err: Optional[BaseException] = None
        self.t = threading.Thread(target=self._run, daemon=True, name=f"cutseq-write-{os.path.basename(path)}")
        self.t.start()

    def put(self, view: memoryview, shared: _Shared) -> None:
        if self.err is not None:
            shared.done()
            raise self.err
        if self.gz and not self.precompressed:
            pool = fastq._pool()
            member = codec.bgzf_blocks if self.bgzf else codec.gzip_member
            futs = [pool.submit(member, view[lo:lo + _GZ_PIECE], self.level) for lo in range(0, len(view), _GZ_PIECE)]
            self.q.put((futs, shared))
        else:
            self.q.put((view, shared))

    def _write_all(self, data) -> None:
        """``data`` at the end of the file.  Writes to ONE file serialise on its inode lock whatever the number of
        threads, so big plain pieces do not go through write(2): the file is extended, the new range mapped, and the
        pool copies into the mapping -- page faults and copies of different pages run side by side."""
        if self.codec is not None:
            data = self.codec[0](data)
        mv = memoryview(data)
        n = len(mv)
        if _DISCARD:  # diagnostic (tools/host_io_profile.py): everything but the writers' copies
            self.pos += n
            return
        if self.stdout:
            at = 0
            while at < n:
                at += os.write(self.fd, mv[at:])
            self.pos += n
            return
        if n >= _MAP_MIN and self.mappable:
            try:
                self._copy_mapped(mv, n)
                self.pos += n
                return
            except (OSError, ValueError, BufferError):
                self.mappable = False  # a file system without usable shared mappings: plain writes from here on
                os.ftruncate(self.fd, self.pos)
        at = 0
        while at < n:
            at += os.pwrite(self.fd, mv[at:], self.pos + at)
        self.pos += n

    def _copy_mapped(self, mv: memoryview, n: int) -> None:
        start, end = self.pos, self.pos + n
        # the new range gets its pages in ONE call where the file system can do that (tmpfs, ext4, xfs: 18 GB/s on the
        # GPU box against 3-6 GB/s when the copies below fault them in one by one; tools/micro/tmpfs_write2.py).
        # Tried again in round 5 and dropped (profiles/r05_host_io.md): allocating the NEXT range meanwhile (fallocate and
        # copies into another range of the same file slow each other down: 16 -> 8 GB/s for two files), and having every
        # copy job map its piece first (madvise MADV_POPULATE_WRITE: +27 % for the writers alone, nothing inside the
        # pipeline, where the same 16 threads also read).
        if not (self._can_allocate and _fallocate(self.fd, start, n)):
            self._can_allocate = False
            os.ftruncate(self.fd, end)
        base = start - start % _PAGE
        mm = mmap.mmap(self.fd, end - base, mmap.MAP_SHARED, mmap.PROT_READ | mmap.PROT_WRITE, offset=base)
        try:
            dst = np.frombuffer(mm, dtype=np.uint8)
            src = np.frombuffer(mv, dtype=np.uint8)
            d0, s0 = dst.ctypes.data + (start - base), src.ctypes.data
            pool = fastq._pool()
            futs = [pool.submit(C.memmove, d0 + lo, s0 + lo, min(_COPY_PIECE, n - lo)) for lo in range(0, n, _COPY_PIECE)]
            for f in futs:
                f.result()
            del dst, src
        finally:
            try:
                mm.close()
            except BufferError:  # (an exception above left a view alive: the mapping goes with the garbage collector)
                pass

    def _run(self):
        while True:
            t0 = time.perf_counter()
            item = self.q.get()
            t0 = _tick("idle", t0)
            if item is None:
                return
            payload, shared = item
            try:
                if self.err is None:
                    if isinstance(payload, list):
                        for f in payload:
                            blob = f.result()
                            t0 = _tick("wait_deflate", t0)
                            self._write_all(blob)
                            t0 = _tick("write", t0)
                    else:
                        self._write_all(payload)
                        _tick("write", t0)
                elif isinstance(payload, list):
                    for f in payload:  # the views must not outlive their buffer
                        try:
                            f.result()
                        except BaseException:
                            pass
            except BaseException as exc:
                self.err = exc
            finally:
                shared.done()

    def close(self) -> None:
        self.q.put(None)
        self.t.join()
        try:
            if self.err is None and self.bgzf:
                self._write_all(codec.BGZF_EOF)  # (an empty output is the marker alone)
            elif self.err is None and self.gz and self.pos == 0:
                self._write_all(codec.gzip_member(b"", self.level))  # an empty stream is still a valid gzip file
            if self.err is None and self.codec is not None:
                tail, self.codec = self.codec[1](), None
                self._write_all(tail)
        finally:
            os.close(self.fd)
        if self.err is not None:
            raise self.err


class _Done:
    __slots__ = ("n", "res", "out", "sizes", "counts", "info", "info_bytes", "discards")

    def __init__(self, n, res, out, sizes=None, counts=None, info=None, info_bytes=0, discards=None):
        self.n, self.res, self.out, self.sizes, self.counts = n, res, out, sizes, counts
        self.discards = discards  # plans with -M / --max-n / --max-ee: pairs (too_long, too_many_n, too_many_ee) took
        self.info, self.info_bytes = info, info_bytes  # --info-file: the batch's table (a pinned buffer) and its size


class TextWorker(fanout.Worker):
    """One GPU.  Counterpart of one worker process of ``make_runner(inpaths, cores=N)`` (cutseq/run.py:436, 753).
    An item is the pair of the mates' blocks ``(b1, b2 | None)``, a finished one a :class:`_Done`."""

    SLOTS = 3
    _tick = staticmethod(_tick)

    def __init__(self, tp, device: int, chunk_reads: int, options: TextOptions):
        super().__init__(f"cutseq-gpu{device}")
        self.tp, self.device, self.chunk_reads, self.options = tp, device, chunk_reads, options
        self.mates_out = 2 if tp.paired and not options.interleave_out else 1  # (a woven route comes back as one stream)
        # --rename: the plan's template as the segments cs_text_set_rename takes (None: the reference's own names)
        self.rename = rename.compile_template(tp.rename, tp) if tp.rename is not None else None
        self.text = None
        self.stride, self.capacity, self.want_stride = 152, 0, 152

    def begin(self):
        # the trimming engine right away (plan upload, code object load: 0.1-0.2 s), while the readers are still
        # getting their first blocks; the text engine follows when the first block says how big it has to be
        from .engine import TrimEngine
        self.engine = TrimEngine(self.tp, device=self.device, slots=0)

    def ensure(self, item):
        """The text engine, rebuilt for longer rows or bigger blocks -- after everything in flight came back."""
        b1, b2 = item
        text_bytes = max(b1.text_size(), b2.text_size() if b2 is not None else 0)
        stride = max(self.stride, self.want_stride)
        if self.text is not None and stride <= self.stride and text_bytes <= self.capacity:
            return
        self.drain()
        if self.text is not None:
            self.text.close()
        self.stride = stride
        self.capacity = max(self.capacity, int(text_bytes * 1.25) + (1 << 20))
        self.text = textpath.TextEngine(self.engine, slots=self.SLOTS, max_text_bytes=self.capacity,
                                        max_records=self.chunk_reads, stride=self.stride, rename=self.rename,
                                        **dataclasses.asdict(self.options))

    def submit(self, slot: int, item):
        b1, b2 = item
        if b1.dbuf is not None or (b2 is not None and b2.dbuf is not None):
            # a reader in device mode: the text is on the device already (a mate that came the host's way is copied by
            # the same call: the copy goes by where each pointer lives)
            self.text.submit_device(slot, b1.text_address(), b1.nbytes, b2.text_address() if b2 is not None else 0,
                                    b2.nbytes if b2 is not None else 0, b1.n)
            return item
        if b1.offsets is not None:  # BAM records: the device expands them to the text (both mates are BAM or none is)
            self.text.submit_bam(slot, b1.buf, b1.nbytes, b1.offsets, b2.buf if b2 is not None else None,
                                 b2.nbytes if b2 is not None else 0, b2.offsets if b2 is not None else None, b1.n)
            return item
        self.text.submit(slot, b1.buf, b1.nbytes, b2.buf if b2 is not None else None, b2.nbytes if b2 is not None else 0, b1.n)
        return item

    def finish(self, slot: int, item) -> _Done:
        b1, b2 = item
        t0 = time.perf_counter()
        try:
            # (a refused BAM record is named by its number in its file: an interleaved block's first record is 2 * its
            # first pair; every other message counts as it does for FASTQ)
            woven_bam = b1.offsets is not None and b2 is None and self.tp.paired
            res = self.text.wait(slot, first_record=b1.first_record, bam_first_record=b1.first_record * (2 if woven_bam else 1))
            t0 = _tick("wait", t0)
        except ReadTooLong as exc:
            raise ReadTooLong(f"{exc} in records {b1.first_record + 1}..{b1.first_record + b1.n}", exc.longest)
        except textpath.TextFormatError as exc:
            if exc.code == abi.CS_TEXT_ERR_IDS_DIFFER:
                raise ValueError(str(exc))
            raise fastq.FastqFormatError(str(exc))
        # Reads longer than the rows took the exact but slow long-read kernel.  A library whose reads are simply longer
        # than the rows so far (2 x 250, 2 x 300) should not stay there: longer rows from the next batch on.
        if max(res.n_long) * 64 > b1.n and self.stride < abi.CS_MAX_STRIDE:
            self.want_stride = max(self.want_stride, min(abi.CS_MAX_STRIDE, (int(res.max_len) + 3) // 4 * 4))
        sizes = counts = None
        if self.options.bins or self.options.too_long_route:
            sizes, _, counts = self.text.routes(slot)
        discards = self.text.discards(slot) if self.tp.has_filters else None
        out = [fastq.PINNED.take(max(int(res.out_bytes[m]), 1)) for m in range(self.mates_out)]
        info_buf, info_bytes = None, 0
        if self.options.info:
            info_bytes = self.text.info(slot)[0]
            info_buf = fastq.PINNED.take(max(info_bytes, 1))
            self.text.fetch_info(slot, info_buf)
        t0 = _tick("take", t0)
        self.text.fetch(slot, out[0], out[1] if self.mates_out == 2 else None)
        _tick("fetch", t0)
        b1.release()
        if b2 is not None:
            b2.release()
        return _Done(b1.n, res, out, sizes, counts, info_buf, info_bytes, discards)

    def close(self):
        try:
            if self.text is not None:
                self.text.close()
        finally:
            if self.engine is not None:
                self.engine.close()


_FASTA_EXT = (".fasta", ".fa", ".fna", ".csfasta", ".csfa")
_FASTQ_EXT = (".fastq", ".fq")


def format_endings(name: str):
    """-> (format extension, compression suffix) of an output file's name as they are written in it, "" where the
    name has none: "x.FA.gz" -> (".FA", ".gz")."""
    low = name.lower()
    container = next((ext for ext in (".gz", ".bz2", ".xz", ".zst") if low.endswith(ext)), "")
    stem = low[: len(low) - len(container)]
    kind = next((ext for ext in _FASTA_EXT + _FASTQ_EXT if stem.endswith(ext)), "")
    return name[len(stem) - len(kind):len(stem)], name[len(stem):]


def format_of_name(name: str) -> Optional[str]:
    """dnaio's rule for output files: the format goes by the extension in front of a compression suffix; None when
    the name says nothing (the input's format then decides)."""
    kind = format_endings(name)[0].lower()
    return "fasta" if kind in _FASTA_EXT else ("fastq" if kind in _FASTQ_EXT else None)


def output_format(names, has_qualities: bool) -> bool:
    """-> True when the records leave as FASTA.  What OutputFiles(qualities=runner.input_file_format().has_qualities())
    does in the reference (cutseq/run.py:437-441, 754-758): a name with a FASTA / FASTQ extension fixes the format,
    any other name follows the input; FASTQ output of an input without qualities is an error (dnaio refuses it)."""
    kinds = {format_of_name(n) or ("fastq" if has_qualities else "fasta") for n in names}
    if "fastq" in kinds and not has_qualities:
        raise fastq.FastqFormatError(
            "Output format cannot be FASTQ since no quality values are available: the input is FASTA "
            "(name the output files .fasta / .fa)")
    if len(kinds) > 1:
        raise ValueError("the output files name different formats (FASTA and FASTQ): one format per run")
    return kinds == {"fasta"}


def output_formats(groups, has_qualities: bool) -> int:
    """-> ``cs_text_params.fasta_routes``: every output file in the format ITS name asks for, as the reference's
    ``OutputFiles.open_record_writer`` hands each name to dnaio on its own (cutseq/run.py:437-441, 449, 465, 754-758).

    ``groups``: the files by the stream they receive -- [trimmed, too short, untrimmed, barcode 0, barcode 1, ...],
    or [trimmed, too short, untrimmed, too long] for a run with ``--too-long-output`` (class 3 as well: such a run has
    no barcodes) --, each a list of names by mate (None / "": no such file), AFTER any swap of the mates' files: the format goes with
    the file.  Bit ``2 * class + mate`` of the result is set when that stream leaves as FASTA; every barcode's files are
    class 3 and must agree per mate (their names come from one template).  Per file the rule of
    :func:`output_format`: a FASTA / FASTQ extension decides, any other name follows the input; a FASTQ file of an
    input without qualities is an error that names the file.

    A stream without a file is formatted and dropped.  It follows the input like a name that says nothing, unless
    every file there is asks for FASTA: then it is FASTA too, so that a run whose files agree stays a run of one
    format on the device (and the dropped records are the shorter ones)."""
    follow = "fastq" if has_qualities else "fasta"
    named = {format_of_name(n) or follow for group in groups for n in list(group)[:2] if n}
    absent = "fasta" if named == {"fasta"} else follow
    mask = 0
    bins = [None, None]  # class 3: the format the first barcode's file of a mate asked for
    for q, group in enumerate(groups):
        for m, name in enumerate(list(group)[:2]):
            kind = (format_of_name(name) or follow) if name else absent
            if kind == "fastq" and not has_qualities:
                raise fastq.FastqFormatError(
                    "Output format cannot be FASTQ since no quality values are available: the input is FASTA "
                    f"and the output file {name!r} is named as FASTQ (name it .fasta / .fa)")
            if q >= 3 and name:
                if bins[m] is not None and bins[m] != kind:
                    raise ValueError(f"the barcodes' output files of mate {m + 1} name different formats "
                                     f"({name!r} is {kind.upper()}): all bins of a mate share one format")
                bins[m] = kind
            if kind == "fasta":
                mask |= 1 << (2 * min(q, 3) + m)
    return mask


def output_name_groups(args, paired: bool, swap_outputs: bool, n_bins: int) -> List[list]:
    """``args.outputs.name_groups(swap_outputs)`` under its name of old (``paired`` and ``n_bins`` are the layout's own)."""
    return args.outputs.name_groups(swap_outputs)


def text_options(layout, tp, fasta: bool, gpu_deflate: bool) -> TextOptions:
    """What the text engines of a run are told: from the output layout, the plan, the input's format (``fasta``: it has
    no qualities) and the CUTSEQ_GPU_DEFLATE switch.
    ``compress``: every output a ".gz" file -- the device compresses (deflate_kernels.hip.inc) and the writers pass the
    members through; otherwise text comes back and ".gz" outputs are deflated in the host pool.  ``info``: the
    --info-file table is one more stream per batch; its container goes by the file's name like a record output's, and a
    ".gz" table leaves the device as gzip members under the same switch.  ``--bgzf`` (``layout.bgzf``): ``compress`` is
    2, the device writes BGZF blocks; a handle has one form for all it compresses, so a ".gz" table beside records the
    host compresses is the host's too."""
    groups = layout.name_groups(tp.swap_outputs)
    names = layout.names(info=False)
    compress = gpu_deflate and bool(names) and all(n != "-" and codec.container_of_name(n) == "gzip" for n in names)
    if compress and layout.bgzf:
        compress = 2
    info = 0
    if layout.info_file:
        info_gz = gpu_deflate and layout.info_file != "-" and codec.container_of_name(layout.info_file) == "gzip"
        if layout.bgzf and not compress:
            info_gz = False
        info = abi.CS_INFO_ON | (abi.CS_INFO_GZIP if info_gz else 0) | (abi.CS_INFO_NO_QUAL if fasta else 0)
    return TextOptions(
        compress=compress,
        bins=len(tp.demux.barcodes) if tp.demux is not None else 0,  # (table form: the pairs of barcode b are route 3 + b)
        # (an interleaved class is one file, hence one format: both mates' bits follow its name)
        fasta_routes=output_formats([g * 2 for g in groups] if layout.interleaved_out else groups, has_qualities=not fasta),
        info=info, too_long_route=layout.too_long_route, interleave_in=layout.interleaved_in,
        interleave_out=layout.interleaved_out, mate2_first=layout.interleaved_out and tp.swap_outputs)


def run_text_pipeline(args, tp, devices, chunk_reads: int, shares=None) -> dict:
    """The CLI's run on the text path -> the run statistics ``report`` expects.  ``shares``: per input file the part
    of it this process takes (``ranks.py``)."""
    global _DISCARD
    _DISCARD = switches.enabled("DISCARD_OUTPUT")  # diagnostic: the writers drop their bytes
    paired = tp.paired
    layout = args.outputs
    # --interleaved: one reader whose blocks hold both mates (2 * chunk_reads records: chunk_reads pairs) and / or one
    # writer per output class, whose stream the device has woven
    woven_in, woven_out = layout.interleaved_in, layout.interleaved_out
    if woven_in and shares is not None:
        raise ValueError("an interleaved input cannot be split between ranks")
    share = shares or [{}, {}]
    make_inflater = None
    if (switches.enabled("GPU_INFLATE") and len(devices) == 1 and shares is None and not woven_in and tp.demux is None):
        # BGZF FASTQ inputs inflate on the device and stay there (each reader decides for its own file)
        def make_inflater():
            from .inflater import DeviceInflater
            return DeviceInflater(devices[0])
        share = [dict(s, inflater=make_inflater) for s in share]
    if woven_in:
        r1 = TextReader(args.input_file[0], 2 * chunk_reads, interleaved=True)
    else:
        r1 = TextReader(args.input_file[0], chunk_reads, **share[0])  # (a missing input file raises here, before anything else exists)
    r2 = None
    opened: List[StreamWriter] = []
    try:
        r2 = TextReader(args.input_file[1], chunk_reads, **share[1]) if paired and not woven_in else None
        report.phase("readers started")

        if r2 is not None and r1.bam != r2.bam:
            raise fastq.FastqFormatError("the two input files are in different formats (one BAM, one FASTQ or FASTA)")
        if r2 is not None and r1.fasta != r2.fasta:
            raise fastq.FastqFormatError("the two input files are in different formats (one FASTA, one FASTQ)")
        if r1.fasta and tp.max_ee is not None:
            raise fastq.FastqFormatError("--max-ee needs qualities: the input is FASTA")
        if r1.fasta and tp.has_nextseq:  # (the qualities the FASTA re-shaper invents would not stop the Gs from going)
            raise fastq.FastqFormatError(f"--nextseq-trim needs qualities: {args.input_file[0]} is a FASTA file.")
        options = text_options(layout, tp, r1.fasta, switches.enabled("GPU_DEFLATE"))

        def writer(name, precompressed):
            opened.append(StreamWriter(name, precompressed=bool(precompressed), bgzf=layout.bgzf))
            return opened[-1]

        outs = [[writer(n, options.compress) if n else None for n in names] for names in layout.name_groups(tp.swap_outputs)]
        info_out = writer(layout.info_file, bool(options.info & abi.CS_INFO_GZIP)) if layout.info_file else None
    except BaseException:
        r1.close()
        if r2 is not None:
            r2.close()
        for fh in opened:
            try:
                fh.close()
            except BaseException:
                pass
        raise
    totals = report.new_totals()
    t_start = time.perf_counter()
    report.phase("readers and writers open")
    workers = [TextWorker(tp, dev, chunk_reads, options) for dev in devices]
    totals["routes"] += [0] * options.bins
    budget = threading.Semaphore(2 * len(workers) * TextWorker.SLOTS + 2)  # batches between reader and disk
    progress = report.Progress()

    def pairs():
        """The mates' blocks, side by side."""
        while True:
            t0 = time.perf_counter()
            b1 = r1.get()
            b2 = r2.get() if r2 is not None else None
            _tick("main_wait_readers", t0)
            if b1 is None and b2 is None:
                return
            if r2 is not None and (b1 is None or b2 is None or b1.n != b2.n):
                for b in (b1, b2):
                    if b is not None:
                        b.release()
                raise fastq.FastqFormatError(
                    "Reads are improperly paired! There are more reads in one file than in the other, "
                    "or a record is truncated.")
            yield b1, b2

    def admit(failed):
        while not budget.acquire(timeout=0.2):
            if failed():
                return

    def emit(item: _Done):
        res = item.res
        totals["in_pairs"] += item.n
        progress.update(item.n)
        if item.counts is not None:  # (demultiplexing: [0] stays 0, the barcodes' pairs are routes 3 ..; a too-long
            for q in range(len(totals["routes"])):  # route is no route of the totals: "too_long" below counts its pairs)
                totals["routes"][q] += int(item.counts[q])
        else:
            for q in range(3):
                totals["routes"][q] += int(res.route_count[q])
        for m in range(2 if paired else 1):
            totals["written_bp"][m] += int(res.written_bp[m])
        if item.discards is not None:
            for key, pairs in zip(("too_long", "too_many_n", "too_many_ee"), item.discards):
                totals[key] += pairs
        sizes = item.sizes if item.sizes is not None else res.route_bytes
        jobs = []
        for m in range(2 if paired and not woven_out else 1):
            at = 0
            for route in range(len(outs)):
                nbytes = int(sizes[route][m])
                fh = (outs[route] + [None])[m]
                if nbytes and fh is not None:
                    jobs.append((fh, memoryview(item.out[m])[at:at + nbytes]))
                at += nbytes
        if info_out is not None and item.info_bytes:
            jobs.append((info_out, memoryview(item.info)[:item.info_bytes]))
        shared = _Shared(item.out + ([item.info] if item.info is not None else []), len(jobs), budget.release)
        for fh, view in jobs:
            fh.put(view, shared)

    def orphan(item: _Done):
        for b in item.out + ([item.info] if item.info is not None else []):
            fastq.PINNED.give(b)
        budget.release()

    def discard(item):
        for b in item:
            if b is not None:
                b.release()

    fanout.run_ordered(workers, pairs(), emit, orphan, admit=admit, discard=discard,
                       closers=[r.close for r in (r1, r2) if r is not None] + [fh.close for fh in opened])
    # (the pinned arena stays: page-locking gigabytes costs more than a short run; it is freed when the process ends)
    stats = [w.stats for w in workers if w.stats is not None]
    for m in range(2 if paired else 1):
        totals["in_bp"][m] = sum(int(pair[m]["in_bp"]) for pair in stats)
        totals["out_bp"][m] = sum(int(pair[m]["out_bp"]) for pair in stats)
    totals["seconds"] = time.perf_counter() - t_start
    progress.close()
    totals["bin_names"] = list(args.demux[0]) if options.bins else None
    totals["stats"] = stats
    if tp.has_poly_a:  # (--poly-a: PolyATrimmer.trimmed_bases per mate; a run without the option has no such key)
        totals["poly_a_bp"] = [sum(w.poly_a_bp[m] for w in workers if w.poly_a_bp is not None) for m in range(2)]
    totals["devices"] = devices
    totals["path"] = "text"
    if PROFILE:
        import json
        import sys
        with _prof_lock:
            print(json.dumps({"cutseq_profile": {k: round(v, 3) for k, v in sorted(_prof.items())},
                              "seconds": round(totals["seconds"], 3), "inflate": dict(_inflate_blocks)}), file=sys.stderr)
            _prof.clear()
            for key in _inflate_blocks:
                _inflate_blocks[key] = 0
    return totals
