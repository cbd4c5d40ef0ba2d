"""Text path of the engine: record-aligned FASTQ text in, finished FASTQ text out (``cs_text_*`` in
``include/cutseq_hip.h``).

Counterpart of what dnaio's reader / writer and the name modifiers do around cutadapt's modifier loop for the
reference (cutseq/run.py:434-441, 751-758 reader; 330, 378, 537-542, 642-645 SuffixRemover / Renamer; 446-471,
760-793 filters and sinks): the device finds the records in the uploaded text, trims them and writes the output
records of the three routes; the host reads / inflates and deflates / writes, nothing else.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import abi, capi
from .abi import ReadTooLong  # noqa: F401  (the name callers know it by)
from .engine import TrimEngine
from .plan import CutOp, TrimPlan

ROUTES = ("trimmed", "short", "untrimmed")


class TextFormatError(ValueError):
    """A record the reference's reader would refuse (malformed FASTQ, mate ids that differ)."""

    def __init__(self, code: int, record: int, message: str):
        super().__init__(message)
        self.code, self.record = code, record


# What a refused BAM record raises ({n}: the record's 0-based number in its file); one sentence per refusal.
BAM_MESSAGES = {
    abi.CS_TEXT_ERR_BAM_BLOCK_SIZE: "malformed BAM: record {n} has a block_size below 32",
    abi.CS_TEXT_ERR_BAM_OVERRUN: "malformed BAM: name, cigar, bases and qualities of record {n} exceed its block_size",
    abi.CS_TEXT_ERR_BAM_NAME: "malformed BAM: the read name of record {n} is empty or lacks its NUL",
    abi.CS_TEXT_ERR_BAM_ALIGNED: "only unaligned BAM is supported: record {n} is aligned",
    abi.CS_TEXT_ERR_BAM_NAME_LINE_END: "malformed BAM: a line end inside the read name of record {n}",
    abi.CS_TEXT_ERR_BAM_NO_QUAL: "BAM record without qualities: record {n}",
    abi.CS_TEXT_ERR_BAM_QUAL_RANGE: "malformed BAM: a quality above 93 in record {n}",
}


class InfoMismatch(RuntimeError):
    """``CS_TEXT_ERR_INFO_MISMATCH`` / ``CS_TEXT_ERR_INFO_OVERFLOW``: an engine fault, never the input's."""


def max_tag(plan: TrimPlan) -> int:
    """Most bytes a record name can gain: '_' + every captured cut (Renamer template, cutseq/run.py:378, 643)."""
    if not plan.has_umi:
        return 0
    total = 1
    for chain in (plan.r1, plan.r2):
        if chain is None:
            continue
        total += sum(abs(op.length) for op in chain.ops if isinstance(op, CutOp) and op.capture)
    return total


_EMPTY = np.zeros(16, dtype=np.uint8)  # stands in for an empty text (a null pointer means "no such mate")


def _address(buf) -> int:
    if buf is None:
        return 0
    if isinstance(buf, int):
        return buf
    if len(buf) == 0:
        return _EMPTY.ctypes.data
    return np.frombuffer(buf, dtype=np.uint8).ctypes.data if not isinstance(buf, np.ndarray) else buf.ctypes.data


class TextEngine:
    """``slots`` batches in flight on one :class:`TrimEngine` (its plan, streams and statistics block)."""

    def __init__(self, engine: TrimEngine, slots: int = 3, max_text_bytes: int = 64 << 20, max_records: int = 1 << 18,
                 stride: int = 152, compress: int = False, bins: int = 0, fasta: bool = False,
                 fasta_routes: int = 0, info: int = 0, too_long_route: bool = False,
                 interleave_in: bool = False, interleave_out: bool = False, mate2_first: bool = False, rename=None):
        """``rename``: a :class:`cutseq_amd.rename.Compiled` -- cutadapt's ``--rename``, every record's name by that template
        (``cs_text_set_rename``) in place of the plan's default; not with ``bins``.
        ``interleave_in`` / ``interleave_out`` / ``mate2_first``: cutadapt's ``--interleaved`` on a paired plan
        (``cs_text_create_interleaved``) -- :meth:`submit` takes ONE text of ``2 * n_records`` records, mate 1 and mate 2
        alternating; every route's two streams leave as one in mate 1's buffer, mate 1's record first (``mate2_first``:
        mate 2's), and the sizes of mate 2's streams are 0.  Not with ``bins``.
        ``too_long_route``: cutadapt's ``--too-long-output`` -- the pairs ``-M`` catches are written as route 3, a
        fourth stream (:meth:`routes`), class 3 of ``fasta_routes``; the plan needs ``max_length`` and no ``bins``.
        ``info``: ``abi.CS_INFO_*`` bits -- the batch also yields cutadapt's ``--info-file`` table for read 1
        (:meth:`info`, :meth:`fetch_info`).  ``compress``: every route's output leaves the device as one gzip member (``res.route_bytes`` then counts
        compressed bytes): what ``.gz`` output files take as they are; 2: as BGZF blocks, one per 32 KB chunk, without the
        EOF marker (``cs_text_params.compress``).  ``bins``: the plan demultiplexes (table form)
        into that many barcodes; the trimmed records of barcode b are route 3 + b (:meth:`routes`).  ``fasta``: every
        record leaves as ``>id\nsequence\n``; ``fasta_routes``: the same per stream, bit ``2 * class + mate`` (class 0
        trimmed, 1 too short, 2 untrimmed, 3 every barcode's route), for output files that name different formats."""
        self.L = capi.load()
        self.engine = engine
        plan = engine.plan
        self.slots, self.max_text_bytes, self.max_records, self.stride = slots, max_text_bytes, max_records, stride
        p = abi.cs_text_params()
        p.has_umi = 1 if plan.has_umi else 0
        p.untrimmed_filter = 1 if plan.untrimmed_filter else 0
        p.reverse_complement = 1 if plan.reverse_complement else 0
        p.compress = 2 if compress == 2 else (1 if compress else 0)
        p.fasta_out = 1 if fasta else 0  # records leave as ">id\nsequence\n" (no qualities to write)
        p.fasta_routes = int(fasta_routes)
        self.compress = bool(compress)
        p.n_bins = int(bins)
        p.info = int(info)
        self.info_flags = int(info)
        p.too_long_route = 1 if too_long_route else 0
        self.n_routes = 3 + int(bins) + (1 if too_long_route else 0)
        p.max_tag = max_tag(plan)
        self._keep = []  # the literals must outlive the call
        for field, chain in (("suffix1", plan.r1), ("suffix2", plan.r2)):
            lits = [s.encode() for s in (chain.name_suffixes if chain is not None else ())][:2]
            self._keep += lits
            arr = getattr(p, field)
            for i, lit in enumerate(lits):
                arr[i] = lit
        self._h = C.c_void_p()
        self.interleave_in, self.interleave_out = bool(interleave_in), bool(interleave_out)
        self.interleave = ((abi.CS_INTERLEAVE_IN if interleave_in else 0) | (abi.CS_INTERLEAVE_OUT if interleave_out else 0)
                           | (abi.CS_INTERLEAVE_OUT_MATE2_FIRST if mate2_first else 0))
        if self.interleave:
            capi.check(self.L.cs_text_create_interleaved(engine._eng_h, C.byref(p), self.interleave, slots, max_text_bytes,
                                                         max_records, stride, C.byref(self._h)))
        else:
            capi.check(self.L.cs_text_create(engine._eng_h, C.byref(p), slots, max_text_bytes, max_records, stride,
                                             C.byref(self._h)))
        if rename is not None:
            _template, segments, literals = rename
            table = (abi.cs_rename_seg * max(len(segments), 1))(*segments)
            rc = self.L.cs_text_set_rename(self._h, table, len(segments), literals, len(literals))
            if rc:
                self.close()
            capi.check(rc)

    def close(self):
        if getattr(self, "_h", None):
            self.L.cs_text_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def submit(self, slot: int, text1, bytes1: int, text2=None, bytes2: int = 0, n_records: int = 0) -> None:
        """Asynchronous.  ``text1`` / ``text2``: buffers (or addresses) holding ``n_records`` complete records each
        (``interleave_in``: ``text1`` alone, ``2 * n_records`` records); they must stay untouched until :meth:`wait`
        returns."""
        capi.check(self.L.cs_text_submit(self._h, slot, _address(text1), bytes1, _address(text2) or None, bytes2, n_records))

    def submit_device(self, slot: int, dtext1: int, bytes1: int, dtext2: int = 0, bytes2: int = 0, n_records: int = 0) -> None:
        """:meth:`submit` for texts that are on the engine's device already (``cs_text_submit_device``): ``dtext1`` /
        ``dtext2`` are device addresses (0: no such mate), complete when the call is made."""
        capi.check(self.L.cs_text_submit_device(self._h, slot, dtext1 or None, bytes1, dtext2 or None, bytes2, n_records))

    def submit_bam(self, slot: int, bam1, bytes1: int, off1, bam2=None, bytes2: int = 0, off2=None,
                   n_records: int = 0) -> None:
        """:meth:`submit` for unaligned BAM records (``cs_text_submit_bam``): ``bam1`` / ``bam2`` hold whole records back
        to back, ``off1`` / ``off2`` (uint32 arrays) their ``n_records + 1`` ascending offsets (``interleave_in``:
        ``2 * n_records + 1`` in ``off1``); the device expands them to the text :meth:`submit` takes."""
        if not hasattr(self.L, "cs_text_submit_bam"):
            raise capi.HipUnavailable("this build of libcutseq_hip.so has no cs_text_submit_bam")
        capi.check(self.L.cs_text_submit_bam(self._h, slot, _address(bam1), bytes1, _address(off1), _address(bam2) or None,
                                             bytes2, _address(off2) or None, n_records))

    def wait(self, slot: int, first_record: int = 0, names=("mate 1", "mate 2"),
             bam_first_record: Optional[int] = None) -> abi.cs_text_result:
        """Blocks until the batch is formatted on the device.  Raises what the reference's reader would raise for a
        bad record.  Reads longer than the rows are not an error: they took the long-read kernel (``res.n_long``).
        ``bam_first_record``: the number in its file of the batch's first BAM record, where that is not
        ``first_record`` (an interleaved text counts two records to a pair); a refused BAM record is named by it."""
        res = abi.cs_text_result()
        capi.check(self.L.cs_text_wait(self._h, slot, C.byref(res)))
        if res.error == abi.CS_TEXT_ERR_TOO_LONG:
            raise ReadTooLong(f"reads longer than {abi.CS_MAX_READ} nt are not supported (a read of {int(res.max_len)} nt)",
                              int(res.max_len))
        if res.error == abi.CS_TEXT_ERR_MALFORMED:
            raise TextFormatError(res.error, first_record + res.error_record,
                                  f"malformed FASTQ record {first_record + res.error_record + 1} "
                                  "(expected '@' header, sequence, '+' line and a quality line of equal length)")
        if res.error == abi.CS_TEXT_ERR_IDS_DIFFER:
            raise TextFormatError(res.error, first_record + res.error_record,
                                  f"Input read IDs not identical in record {first_record + res.error_record + 1}")
        if res.error == abi.CS_TEXT_ERR_LINE_COUNT:
            raise TextFormatError(res.error, first_record,
                                  f"the text block does not hold the announced number of records ({res.n_records} records, "
                                  f"{res.n_lines[0]} / {res.n_lines[1]} line ends)")
        if (res.error & ~abi.CS_TEXT_ERR_BAM_MATE2) in BAM_MESSAGES:
            record = (first_record if bam_first_record is None else bam_first_record) + res.error_record
            mate = names[1 if res.error & abi.CS_TEXT_ERR_BAM_MATE2 else 0]
            text = BAM_MESSAGES[res.error & ~abi.CS_TEXT_ERR_BAM_MATE2].format(n=record)
            raise TextFormatError(res.error, record, f"{mate}: {text}")
        if res.error == abi.CS_TEXT_ERR_INFO_MISMATCH:
            raise InfoMismatch(f"--info-file: the match recorder and the trimming kernels disagree on record "
                               f"{first_record + res.error_record + 1}; no table is written for a batch that "
                               "contradicts its records")
        if res.error == abi.CS_TEXT_ERR_INFO_OVERFLOW:
            raise InfoMismatch("--info-file: the table of a block outgrew the buffer sized for it "
                               f"(records {first_record + 1}..{first_record + res.n_records})")
        return res

    def info(self, slot: int):
        """Behind :meth:`wait`, before :meth:`fetch`: (bytes as :meth:`fetch_info` delivers them, text bytes, rows) of
        the batch's info table."""
        got, raw, rows = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        capi.check(self.L.cs_text_info(self._h, slot, C.byref(got), C.byref(raw), C.byref(rows)))
        return int(got.value), int(raw.value), int(rows.value)

    def fetch_info(self, slot: int, dst) -> None:
        """The info table (a gzip member with ``CS_INFO_GZIP``) into ``dst``; the slot stays taken until :meth:`fetch`."""
        capi.check(self.L.cs_text_fetch_info(self._h, slot, _address(dst) or None))

    def routes(self, slot: int):
        """Behind :meth:`wait`: (bytes[route, mate] as fetched, text_bytes[route, mate], count[route]) of every route."""
        got = np.zeros((self.n_routes, 2), dtype=np.uint64)
        raw = np.zeros((self.n_routes, 2), dtype=np.uint64)
        count = np.zeros(self.n_routes, dtype=np.uint32)
        capi.check(self.L.cs_text_routes(self._h, slot, got.ctypes.data, raw.ctypes.data, count.ctypes.data))
        return got, raw, count

    def discards(self, slot: int):
        """Behind :meth:`wait`: the batch's pairs that (too_long, too_many_n, too_many_ee) discarded, each pair under
        the first of the three filters that caught it."""
        pairs = (C.c_uint32 * 3)()
        capi.check(self.L.cs_text_discards(self._h, slot, C.byref(pairs)))
        return int(pairs[0]), int(pairs[1]), int(pairs[2])

    def fetch(self, slot: int, dst1, dst2=None) -> None:
        """Output text of the batch into the caller's buffers (``res.out_bytes[m]`` bytes each); frees the slot."""
        capi.check(self.L.cs_text_fetch(self._h, slot, _address(dst1) or None, _address(dst2) or None))

    def run(self, text1: bytes, n_records: int, text2: Optional[bytes] = None, slot: int = 0):
        """Synchronous convenience wrapper (tests): -> (streams[route][mate] bytes, counts[route])."""
        self.submit(slot, text1, len(text1), text2, len(text2) if text2 is not None else 0, n_records)
        res = self.wait(slot)
        got, _, count = self.routes(slot)
        paired = text2 is not None or self.interleave_in
        out = [np.empty(max(int(res.out_bytes[m]), 1), dtype=np.uint8) for m in range(2)]
        self.fetch(slot, out[0], out[1] if paired and not self.interleave_out else None)
        if self.n_routes > 3:
            return split_routes(got, out, paired), [int(c) for c in count]
        return split_routes(res, out, paired), [int(c) for c in res.route_count]


def split_routes(res, out, paired: bool):
    """-> streams[route][mate] (bytes) from the per-mate buffers :meth:`TextEngine.fetch` filled.  ``res``: the
    ``cs_text_result`` of the batch, or the bytes[route, mate] array of :meth:`TextEngine.routes`.  An interleaved
    output (``interleave_out``) has sizes of 0 for mate 2: every route comes back as ``[woven stream, b""]``."""
    sizes = res.route_bytes if isinstance(res, abi.cs_text_result) else res
    streams = [[b"", b""] for _ in range(len(sizes))]
    for m in range(2 if paired else 1):
        at = 0
        for route in range(len(sizes)):
            n = int(sizes[route][m])
            streams[route][m] = out[m][at:at + n].tobytes()
            at += n
    return streams
