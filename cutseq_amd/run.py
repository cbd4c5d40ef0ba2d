#!/usr/bin/env python3
"""cutseq-compatible command line on top of the HIP trimming engine.

Rewritten counterpart of the reference's ``cutseq/run.py``: same flags (run.py:874-1020), same
preset resolution and upper-casing (1041-1056), same output naming (1058-1107), same single /
paired dispatch (842-863).  Where the reference assembles cutadapt modifiers and calls
``runner.run``, this compiles the op table (``plan.compile_*``) and streams record-aligned FASTQ
chunks through :class:`cutseq_amd.engine.TrimEngine` (one per visible GPU, chunks round-robin,
ordered write-back).  ``-t/--threads`` bounds the host thread pool that parses, formats and (de)compresses
(the reference passes it to ``make_runner(cores=N)``, run.py:436, 753); the per-read work runs on the GPU(s).
"""
from __future__ import annotations

import argparse
import itertools
import logging
import os
import re
import sys
import time
from collections import deque
from typing import List, Optional

from . import __version__, abi, fanout, outputs, rename, report, switches
from .abi import ReadTooLong
from .common import BUILDIN_ADAPTERS, BarcodeConfig, print_builtin_adapters
from .outputs import OUTPUT_CLASSES, _fail  # noqa: F401 -- (OUTPUT_CLASSES: under the name it had here)
from .plan import CutadaptConfig, TrimPlan, compile_paired, compile_single
from .report import phase as _phase

logging.basicConfig(level=logging.INFO, format="%(asctime)s -  %(levelname)s - %(message)s")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog="cutseq",
        description="Trim sequencing adapters from NGS data automatically (MI355X-native engine, cutseq-compatible CLI).",
    )
    p.add_argument("input_file", type=str, nargs="*",
                   help="Input file path for NGS data, one or two files (for single or paired-end reads).")
    p.add_argument("-a", "--adapter-scheme", type=str,
                   help="Adapter sequence configuration string. Example: P5(INLINE5)UMI5XXXS>P7(INLINE3)UMI3XXXS. "
                        "Where P5/P7 are adapter sequences, (INLINE5/3) are optional inline barcodes, "
                        "UMI5/3 are N's for UMI bases, XXX are mask sequences, S is strand (>/< or -).")
    p.add_argument("-A", "--adapter-name", help="Built-in adapter name. choices:\n" + ",".join(BUILDIN_ADAPTERS.keys()))
    p.add_argument("-O", "--output-prefix", type=str,
                   help="Output file prefix for trimmed, short, and untrimmed data. "
                        "If not provided, output filenames are derived from input filenames.")
    p.add_argument("-o", "--output-file", type=str, nargs="+",
                   help="Output file path(s) for successfully trimmed reads. Must match number of input files.")
    p.add_argument("-s", "--short-file", type=str, nargs="+",
                   help="Output file path(s) for reads discarded due to being too short after trimming.")
    p.add_argument("-u", "--untrimmed-file", type=str, nargs="+",
                   help="Output file path(s) for reads discarded because expected inline barcodes were not found.")
    p.add_argument("--json-file", type=str, help="Output JSON file for trimming statistics.")
    p.add_argument("-q", "--min-quality", action=_QualityCutoffs, default=20, metavar="[5'CUTOFF,]3'CUTOFF",
                   help="Minimum quality score for trimming read tails. (Default: 20) Extension (cutadapt's form of "
                        "the option): two values separated by a comma trim the 5' end with the first cutoff and the "
                        "3' end with the second.")
    p.add_argument("-Q", dest="min_quality_r2", action=_QualityCutoffs, default=None, metavar="[5'CUTOFF,]3'CUTOFF",
                   help="Extension (cutadapt's option): quality-trimming cutoff(s) for the second read of a pair, in the "
                        "form -q takes. (Default: the second read follows -q)")
    p.set_defaults(min_quality_front=0, min_quality_front_r2=None)
    p.add_argument("--nextseq-trim", type=int, default=None, metavar="3'CUTOFF",
                   help="Extension (cutadapt's option): NextSeq/NovaSeq-specific quality trimming of the 3' end, in front "
                        "of -q's: the same walk with this cutoff, in which a G counts as a base of quality CUTOFF - 1 "
                        "whatever its quality value says (the dark cycles of two-colour instruments read as high-quality "
                        "G). Needs an input with qualities.")
    p.add_argument("-l", "--length", type=int, default=None, metavar="LENGTH",
                   help="Extension (cutadapt's option): shorten reads to LENGTH bases, behind adapter and quality "
                        "trimming and in front of --trim-n and the filters. A positive value keeps the first LENGTH "
                        "bases, a negative one the last. Applies to both reads of a pair unless -L is given.")
    p.add_argument("-L", dest="length_r2", type=int, default=None, metavar="LENGTH",
                   help="Extension (cutadapt's option): shorten the second read of a pair to LENGTH, in the form -l "
                        "takes. (Default: the second read follows -l)")
    p.add_argument("-m", "--min-length", type=int, default=20,
                   help="Minimum length of reads to keep after trimming. (Default: 20)")
    p.add_argument("--with-rname-suffix", action="store_true",
                   help="Indicate if read names have MGI-style suffixes like '/1', '/2', '.1', or '.2' to be stripped.")
    p.add_argument("--ensure-inline-barcode", action="store_true",
                   help="If set, reads without the specified inline barcode(s) will be written to the untrimmed files.")
    p.add_argument("--trim-polyA", action="store_true", help="Enable trimming of polyA/T tails.")
    p.add_argument("--trim-polyA-wo-direction", action="store_true",
                   help="Trim polyA/T tails regardless of strand information.")
    p.add_argument("--poly-a", dest="poly_a", action="store_true",
                   help="Extension (cutadapt's option, cutadapt >= 4.4): trim poly-A tails with cutadapt's own poly-A "
                        "trimmer, which its manual recommends over an adapter of A's: a scored walk from the read's end "
                        "that allows one foreign base in five and ignores tails shorter than three. It stands where "
                        "--trim-polyA's adapters stand; on a (+) library read 1 loses a poly-A tail and read 2 a poly-T "
                        "head, on a (-) library the other way round, without strand information as on (+). Not with "
                        "--trim-polyA.")
    p.add_argument("--conditional-cutter", action=argparse.BooleanOptionalAction, default=True,
                   help="Enable/disable conditional cutting for UMIs/masks.")
    p.add_argument("--force-trim-min-length", type=int, default=50,
                   help="Minimum read length to enforce UMI/mask trimming even if no adapter is found. (Default: 50)")
    p.add_argument("--force-anywhere", action="store_true",
                   help="Force adapter trimming to match anywhere in the read, not just at the ends.")
    p.add_argument("--auto-rc", action="store_true",
                   help="Automatically reverse complement reads if the library strand is '-'. "
                        "For paired-end, R1 and R2 will be swapped.")
    p.add_argument("-t", "--threads", type=int, default=None,
                   help="Number of host threads for reading, (de)compression and writing. The reference's -t "
                        "(default 1) is the number of cutadapt worker PROCESSES that do the per-read work; here that "
                        "work runs on the GPU(s), so -t only bounds the host I/O pool and the output does not depend "
                        "on it. -t 1 is accepted and means one host thread. (Default: all usable cores)")
    p.add_argument("-n", "--dry-run", action="store_true",
                   help="Print the sequence of modifier steps instead of running the pipeline.")
    p.add_argument("-V", "--version", action="version", version=f"%(prog)s {__version__}")
    p.add_argument("--list-adapters", action="store_true",
                   help="List all built-in adapter names and their schemes, then exit.")
    p.add_argument("--cutadapt-selection", choices=["4", "3"], default="4",
                   help="Aligner candidate selection to follow: cutadapt >= 4 (default) or 3.x (DESIGN.md section 0).")
    p.add_argument("--ranks", type=int, default=1, metavar="N",
                   help="Extension: one process per GPU (N processes, rank r on GPU r or on the r-th entry of "
                        "CUTSEQ_DEVICES); the input is split at record boundaries, the output parts are concatenated "
                        "in rank order. Output is identical to the one-process run.")
    p.add_argument("--max-n", type=float, default=None, metavar="COUNT",
                   help="Extension (cutadapt's option; a TODO of the reference): discard reads with more than COUNT 'N' "
                        "bases. If COUNT is a number between 0 and 1, it is interpreted as a fraction of the read "
                        "length. A pair is discarded if either read has too many N.")
    p.add_argument("-M", "--max-length", type=int, default=None, metavar="LEN",
                   help="Extension (cutadapt's option): discard reads longer than LEN after trimming. A pair is discarded "
                        "if either read is too long. The counterpart of -m.")
    p.add_argument("--too-long-output", dest="too_long_file", type=str, nargs="+", metavar="FILE",
                   help="Extension (cutadapt's option): write the reads -M/--max-length catches to FILE (one per input "
                        "file) instead of discarding them: as trimmed, like the too-short files. Needs -M; not with "
                        "--demux-barcodes.")
    p.add_argument("--max-ee", "--max-expected-errors", dest="max_ee", type=float, default=None, metavar="ERRORS",
                   help="Extension (cutadapt's option): discard reads whose expected number of errors, the sum of "
                        "10^(-Q/10) over the trimmed read's qualities, exceeds ERRORS. A pair is discarded if either "
                        "read has too many. Needs an input with qualities.")
    p.add_argument("--trim-n", action="store_true",
                   help="Extension (cutadapt's option): trim N's at both ends of the reads, after adapter and quality "
                        "trimming and before the length and N filters.")
    p.add_argument("--info-file", type=str, default=None, metavar="FILE",
                   help="Extension (cutadapt's option; a TODO of the reference): write a tab-separated table of the "
                        "adapter matches of read 1 to FILE, one row per match, in input order; reads without a match "
                        "get one row with -1. A .gz / .bz2 / .xz / .zst name compresses the table.")
    p.add_argument("--rename", type=str, default=None, metavar="TEMPLATE",
                   help="Extension (cutadapt's option): name every output record by TEMPLATE instead of the default "
                        "('{id}', with a UMI '{id}_{cut_prefix}{cut_suffix}' or, paired, "
                        "'{id}_{r1.cut_prefix}{r2.cut_prefix}'). Placeholders: {header}, {id}, {comment}; single-end "
                        "{cut_prefix}, {cut_suffix}; paired {rn}, {cut_prefix}, {r1.cut_prefix}, {r2.cut_prefix}. "
                        "'{{' and '}}' are braces, '\\t' is a TAB. Example: '{id} RX:Z:{r1.cut_prefix}{r2.cut_prefix}'. "
                        "Not with --demux-barcodes.")
    p.add_argument("--interleaved", action="store_true",
                   help="Extension (cutadapt's option): paired reads in ONE file, mate 1 and mate 2 alternating. With one "
                        "input file, that file holds interleaved pairs (the run is a paired run); the outputs are "
                        "interleaved too unless -o names two files. With two input files, the outputs are interleaved "
                        "(-o takes one name). An interleaved run takes one name each for -o, -s, -u and "
                        "--too-long-output; '-' reads standard input / writes standard output. Not with "
                        "--demux-barcodes.")
    p.add_argument("--bgzf", action="store_true",
                   help="Extension: write every output whose name ends in .gz (-o, -s, -u, --too-long-output, the -O "
                        "defaults, the barcodes' files, --info-file) as BGZF, htslib's blocked form of gzip: any gzip "
                        "reader takes it, bgzip -r / tabix / samtools and this tool (CUTSEQ_GPU_INFLATE=1) get random "
                        "access and parallel decoding. Blocks of 32 KiB of text, laid out on the GPU; the file ends "
                        "with the BGZF EOF marker. Other outputs are untouched. Refused when no output is a .gz file "
                        "and with CUTSEQ_TEXT_PATH=0.")
    p.add_argument("--rank-spec", type=str, help=argparse.SUPPRESS)  # a child of --ranks: its share of the run
    p.add_argument("--demux-barcodes", type=str, metavar="FILE",
                   help="Extension: demultiplex on the 5' inline barcode. FILE lists 'name<TAB>sequence' per line (all as "
                        "long as the scheme's inline barcode); trimmed reads go to <prefix>_<name>_trimmed_R1/2.fastq.gz, "
                        "reads without any of the barcodes to the untrimmed files. Equals one --ensure-inline-barcode "
                        "run per barcode.")
    return p


class _QualityCutoffs(argparse.Action):
    """``-q BACK`` or ``-q FRONT,BACK`` (cutadapt's ``-q [5'CUTOFF,]3'CUTOFF``): ``min_quality`` stays the 3' int, the 5'
    value goes to ``min_quality_front``.  Anything else is an argparse error, like a non-integer was before.  ``-Q``, the
    same for the second read of a pair, fills ``min_quality_r2`` / ``min_quality_front_r2``."""

    def __call__(self, parser, namespace, values, option_string=None):
        parts = values.split(",")
        try:
            cutoffs = [int(part) for part in parts]
        except ValueError:
            raise argparse.ArgumentError(self, f"invalid int value: {values!r}")
        if len(cutoffs) > 2:
            raise argparse.ArgumentError(self, f"expected one value or two separated by a comma: {values!r}")
        # (-q: min_quality / min_quality_front; -Q: min_quality_r2 / min_quality_front_r2)
        front = self.dest.replace("min_quality", "min_quality_front")
        setattr(namespace, self.dest, cutoffs[-1])
        setattr(namespace, front, cutoffs[0] if len(cutoffs) == 2 else 0)


_SCHEME_HAS_INLINE = re.compile(r".*\([ATGCatgc]+\).*")


def resolve_interleaved(args, inputs):
    """``--interleaved`` -> (the input is interleaved, the outputs are).  One input file: it holds the pairs, and the
    outputs are interleaved unless -o names two files.  Two input files: the outputs are interleaved, and -o takes one
    name."""
    if not args.interleaved or not inputs:
        return False, False
    if args.demux_barcodes:
        _fail("--interleaved cannot be combined with --demux-barcodes: the barcodes' kernels write one stream per mate.")
    if not switches.enabled("TEXT_PATH"):
        _fail("--interleaved needs the text path: the pairs are woven on the GPU (CUTSEQ_TEXT_PATH=0 is set).")
    given = len(args.output_file) if args.output_file else 0
    if len(inputs) == 1:
        if args.ranks > 1 and not args.rank_spec:
            _fail("--interleaved input cannot be split between --ranks: a share that begins at a record boundary "
                  "cannot know which mate it begins with (two input files with --interleaved output can).")
        return True, given != 2
    if given == 2:
        _fail("--interleaved with two input files and two -o files would have nothing to do: give -o one name "
              "(interleaved output) or drop --interleaved.")
    return False, True


def resolve_scheme(args) -> str:
    """-a wins over -A; -A looks the preset up case-insensitively and, like the reference, falls back to
    reading an unknown name as a scheme (run.py:1041-1056)."""
    scheme = args.adapter_scheme
    if args.adapter_name is not None and scheme is not None:
        logging.info("Adapter scheme is provided, ignoring adapter name.")
    elif args.adapter_name is not None:
        scheme = BUILDIN_ADAPTERS.get(args.adapter_name.upper())
        if scheme is None:
            logging.error(f"Adapter name '{args.adapter_name} not found in built-in adapters.")
            scheme = args.adapter_name
    if scheme is None:
        _fail("Adapter scheme or name is required. Use -a or -A.")
    return scheme.replace(" ", "").upper()


def resolve_args(args):
    """What the reference's main() settles between parse_args and run_cutseq (run.py:1029-1107)."""
    if args.list_adapters:
        print_builtin_adapters()
        sys.exit(0)
    inputs = args.input_file or []
    if len(inputs) > 2:
        _fail("Input file can not be more than two.")
    args.adapter_scheme = resolve_scheme(args)
    if args.max_n is not None and not args.max_n >= 0:  # (NaN fails the comparison too)
        _fail(f"--max-n: the count must not be negative (got {args.max_n}).")
    if args.max_length is not None and args.max_length < 0:
        _fail(f"-M/--max-length: the length must not be negative (got {args.max_length}).")
    if args.max_ee is not None and not args.max_ee >= 0:  # (NaN fails the comparison too)
        _fail(f"--max-ee: the number of expected errors must not be negative (got {args.max_ee}).")
    nextseq = args.nextseq_trim
    if nextseq is not None and not abi.CS_Q_SUM_LOW <= nextseq + 33 <= abi.CS_Q_SUM_HIGH:
        # (unlike -q's, this cutoff is not clamped: a G's term is +1 whatever it is -- include/cutseq_hip.h, CS_OP_NEXTSEQ)
        _fail(f"--nextseq-trim: the cutoff must lie in [{abi.CS_Q_SUM_LOW - 33}, {abi.CS_Q_SUM_HIGH - 33}] (got {nextseq}).")
    if args.poly_a and args.trim_polyA:
        _fail("--poly-a cannot be combined with --trim-polyA: they are two poly-A trimmers at one step, use one of them.")
    interleaved_in, interleaved_out = resolve_interleaved(args, inputs)
    if args.min_quality_r2 is not None and len(inputs) == 1 and not interleaved_in:
        _fail("-Q sets the quality cutoff of the second read: it needs two input files.")
    if args.length_r2 is not None and len(inputs) == 1 and not interleaved_in:
        _fail("-L shortens the second read: it needs two input files, or one with --interleaved.")
    for option, value in (("-l/--length", args.length), ("-L", args.length_r2)):
        if value is not None and not -2 ** 31 <= value < 2 ** 31:
            _fail(f"{option}: the length must fit 32 bits (got {value}).")
    if args.info_file:
        if args.demux_barcodes:
            _fail("--info-file cannot be combined with --demux-barcodes: the table form of the demultiplexing op has "
                  "no error count to report.")
        if not switches.enabled("TEXT_PATH"):
            _fail("--info-file needs the text path: the table is written on the GPU (CUTSEQ_TEXT_PATH=0 is set).")
    if args.rename is not None:
        if args.demux_barcodes:
            _fail("--rename cannot be combined with --demux-barcodes: the barcodes' kernels write the default names.")
        if not switches.enabled("TEXT_PATH"):
            _fail("--rename needs the text path: the names are built on the GPU (CUTSEQ_TEXT_PATH=0 is set).")
        try:
            rename.check(args.rename, len(inputs) == 2 or interleaved_in or interleaved_out)
        except ValueError as exc:
            _fail(str(exc))
    if args.too_long_file:
        if args.max_length is None:
            _fail("--too-long-output needs -M/--max-length: without it no read is too long.")
        if args.demux_barcodes:
            _fail("--too-long-output cannot be combined with --demux-barcodes: the output class it would take on the "
                  "GPU is the barcodes' there.")
    if not inputs:
        # the reference dies with an IndexError here (run.py:1079-1083); same exit class, clearer message
        _fail("Input file is required.")
    args.demux = None
    if args.demux_barcodes:
        from .demux import read_barcode_file
        if args.output_file:
            _fail("--demux-barcodes names the trimmed files itself (<prefix>_<name>_trimmed_R1.fastq.gz): drop -o.")
        try:
            args.demux = read_barcode_file(args.demux_barcodes)  # ([names], [sequences])
        except (OSError, ValueError) as exc:
            _fail(str(exc))
    wants_untrimmed = bool(args.untrimmed_file) or args.demux is not None or (
        args.ensure_inline_barcode and _SCHEME_HAS_INLINE.match(args.adapter_scheme) is not None)
    layout = args.outputs = outputs.resolve(args, interleaved_in, interleaved_out, wants_untrimmed)
    # (what the options resolved to, for callers that look: nothing in this package reads them from here on)
    args.paired, args.interleaved_in, args.interleaved_out = layout.paired, interleaved_in, interleaved_out
    if layout.bgzf:
        from . import codec
        if not switches.enabled("TEXT_PATH"):
            _fail("--bgzf needs the text path: the blocks are laid out on the GPU and closed by the text path's writers "
                  "(CUTSEQ_TEXT_PATH=0 is set).")
        if not any(n != "-" and codec.container_of_name(n) == "gzip" for n in layout.names()):
            _fail("--bgzf: no output of this run is a gzip file (BGZF is a form of gzip: it goes by the .gz in an "
                  "output's name), so the option would change nothing.")
    for cls in layout.classes:
        if not cls.barcode:
            setattr(args, cls.key, list(cls.names))
    return args


def settings_from_args(args) -> CutadaptConfig:
    st = CutadaptConfig()
    st.rname_suffix = args.with_rname_suffix  # parsed, stored, never consulted (as in the reference)
    st.ensure_inline_barcode = args.ensure_inline_barcode
    st.trim_polyA = args.trim_polyA
    st.trim_polyA_wo_direction = args.trim_polyA_wo_direction
    st.conditional_cutter = args.conditional_cutter
    st.threads = args.threads if args.threads is not None else 0
    st.min_length = args.min_length
    st.min_quality = args.min_quality
    st.min_quality_front = args.min_quality_front
    st.trim_n = args.trim_n
    st.nextseq_trim = args.nextseq_trim
    st.min_quality_r2 = args.min_quality_r2
    st.min_quality_front_r2 = args.min_quality_front_r2
    st.length = args.length
    st.length_r2 = args.length_r2
    st.rename = args.rename
    st.poly_a = args.poly_a
    st.dry_run = args.dry_run
    st.auto_rc = args.auto_rc
    st.json_file = args.json_file
    st.force_trim_min_length = args.force_trim_min_length
    st.force_anywhere = args.force_anywhere
    st.select_rule = abi.CS_SELECT_LEFTMOST if args.cutadapt_selection == "4" else abi.CS_SELECT_SCORE
    st.max_n = args.max_n
    st.max_length = args.max_length
    st.max_ee = args.max_ee
    if args.demux is not None:
        st.demux_barcodes = list(args.demux[1])
    return st


def compile_plan(args, barcode: BarcodeConfig, settings: CutadaptConfig) -> TrimPlan:
    compile_for = compile_paired if args.outputs.paired else compile_single  # (--interleaved: one input file can hold pairs)
    return compile_for(barcode, settings, untrimmed_requested=args.outputs.untrimmed_requested)


def dry_run_steps(tp: TrimPlan) -> List[str]:
    """The reference's modifier list in ITS order (cutseq/run.py:326-426, 533-731): the two SuffixRemovers, the
    adapter and UMI steps, the (PairedEnd)Renamer right behind the UMI step (run.py:377-380, 642-645), then masks,
    poly-A, quality trimming (and the single-end reverse complement).  The text of a step is this build's own
    (cutadapt's ``repr``s are not available here); the ORDER is the reference's."""
    template = tp.rename if tp.rename is not None else rename.default_template(tp.has_umi, tp.paired)
    if tp.paired:
        # (-L without -l: mate 2's chain ends one step behind mate 1's, which has None there)
        steps = [f"({a}, {b})" for a, b in itertools.zip_longest(tp.r1.describe(), tp.r2.describe(), fillvalue="None")]
        renamer = f"PairedEndRenamer({template!r})"
    else:
        steps = list(tp.r1.describe())
        renamer = f"Renamer({template!r})"
    at = len(tp.r1.ops) if tp.r1.rename_at is None else tp.r1.rename_at
    steps.insert(len(tp.r1.name_suffixes) + at, renamer)
    if not tp.paired and tp.reverse_complement:
        steps.append("ReverseComplementConverter()")
    return steps


def dry_run(tp: TrimPlan, barcode: BarcodeConfig):
    if tp.paired:  # run.py:734-749: the parts through print, the steps through logging
        for b in ["p5", "p7", "inline5", "inline3", "umi5", "umi3", "mask5", "mask3", "strand"]:
            print(f"{b}: {getattr(barcode, b)}")
        for i, step in enumerate(dry_run_steps(tp), 1):
            logging.info(f"Step {i}: {step}")
    else:  # run.py:429-432
        for i, step in enumerate(dry_run_steps(tp), 1):
            print(f"Step {i}: {step}")


class _DeviceWorker(fanout.Worker):
    """One GPU: owns the device's TrimEngine, keeps ``SLOTS`` chunks in flight on it (the H2D copy of one
    overlaps the kernels and the D2H copy of the other) and reports every finished chunk to ``done``.
    Counterpart of one worker process of ``make_runner(inpaths, cores=N)`` (cutseq/run.py:436, 753)."""

    SLOTS = 2

    def __init__(self, tp: TrimPlan, device: int, chunk_reads: int):
        super().__init__(f"cutseq-gpu{device}")
        self.tp, self.device, self.chunk_reads = tp, device, chunk_reads
        self.stride_cap = 0

    def ensure(self, chunk):
        """The engine, rebuilt with longer rows when a chunk needs them -- after everything the old one still
        has in flight came back and its counters were saved."""
        if self.engine is not None and chunk.stride <= self.stride_cap:
            return
        from .engine import TrimEngine
        self.drain()
        if self.engine is not None:
            self._collect_stats()
            self.engine.close()
        self.stride_cap = max(chunk.stride, 152)
        self.engine = TrimEngine(self.tp, device=self.device, slots=self.SLOTS, max_reads=self.chunk_reads,
                                 max_stride=self.stride_cap)

    def submit(self, slot: int, chunk):
        from . import fastq
        paired = chunk.paired
        # result arrays in pinned memory, like the inputs: the D2H copy is a DMA transfer too
        owned = [fastq.PINNED.take(chunk.n * 8)]
        out1 = owned[0][: chunk.n * 8].view(abi.RESULT_DTYPE)
        cap2 = out2 = None
        if self.tp.needs_cap2:
            owned.append(fastq.PINNED.take(chunk.n * 4))
            cap2 = owned[-1][: chunk.n * 4].view(abi.CAP2_DTYPE)
        if paired:
            owned.append(fastq.PINNED.take(chunk.n * 8))
            out2 = owned[-1][: chunk.n * 8].view(abi.RESULT_DTYPE)
        if self.tp.demux is not None:
            owned.append(fastq.PINNED.take(chunk.n))
            chunk.bc = owned[-1][: chunk.n]
        if self.tp.has_filters:  # the CS_X_* flags of both mates
            owned.append(fastq.PINNED.take(chunk.n))
            xf1 = owned[-1][: chunk.n]
            xf2 = None
            if paired:
                owned.append(fastq.PINNED.take(chunk.n))
                xf2 = owned[-1][: chunk.n]
            chunk.xflags = (xf1, xf2)
        chunk._owned = chunk._owned + tuple((fastq.PINNED, b) for b in owned)
        res = self.engine.submit(slot, chunk.seq1, chunk.qual1, chunk.len1, chunk.seq2, chunk.qual2,
                                 chunk.len2, out=(out1, cap2, out2), bc=chunk.bc, xflags=chunk.xflags)
        return chunk, res

    def finish(self, slot: int, handle):
        self.engine.wait(slot)
        return handle  # (chunk, result arrays)

    def close(self):
        if self.engine is not None:
            self.engine.close()


def run_pipeline(args, tp: TrimPlan, shares=None) -> dict:
    """Stream the input through the GPU engine(s); returns the run statistics.

    Counterpart of ``runner.run(pipeline, Progress(), outfiles)`` (cutseq/run.py:473, 794): chunks of
    ``fastq.CHUNK_READS`` records go round-robin to one worker thread per GPU, come back in any order and are
    formatted / compressed / written strictly in input order (``fanout.run_ordered``)."""
    from . import capi, fastq

    if args.outputs.bgzf and not switches.enabled("TEXT_PATH"):
        # (resolve_args refuses this; a caller that flips the switch behind it must not get plain gzip members from
        # fastq.py's writers under --bgzf)
        _fail("--bgzf: the record path's writers (CUTSEQ_TEXT_PATH=0) write plain gzip members, not BGZF.")
    n_dev = capi.device_count()
    _phase("devices counted")
    if n_dev <= 0:
        raise capi.HipUnavailable("no HIP device visible; cutseq_amd has no CPU trimming path")
    if args.threads is not None:
        if args.threads < 1:
            _fail("-t/--threads must be at least 1.")
        try:
            fastq.set_threads(args.threads)
        except RuntimeError:  # a second run in one process (tests): the pool of the first run stays
            logging.warning("-t/--threads ignored: the host thread pool of this process is already running.")
    devices = switches.device_list("DEVICES", n_dev)  # e.g. "0,1,2,3"; a device may be listed twice (two engines on it)
    if any(d < 0 or d >= n_dev for d in devices):
        _fail(f"GPU {max(devices)} does not exist: this process sees {n_dev} (--ranks N puts rank r on GPU r; "
              "CUTSEQ_DEVICES=0,0,... lists the GPUs to use, one entry per rank or worker, repeats allowed).")
    # Text path (default): the device parses the records and formats the output (textio.py / cs_text_*), demultiplexing
    # runs included.  The record path below is the second host implementation (native parser / formatter of
    # cutseq_host.c in a thread pool), selected by CUTSEQ_TEXT_PATH=0 and held to the same outputs by the tests.
    from . import textio
    if switches.enabled("TEXT_PATH"):
        return textio.run_text_pipeline(args, tp, devices, _block_records(args, len(devices)),
                                        shares=shares)
    if shares is not None:
        raise ValueError("--ranks needs the text path (no demultiplexing, CUTSEQ_TEXT_PATH unset)")
    from . import codec
    for name in args.input_file:  # the host parser reads plain and gzip FASTQ files, nothing else
        container, first, _ = codec.sniff_input(name) if name != "-" else ("stdin", b"", None)
        if container not in ("plain", "gzip") or first[:1] in (b">", b"#"):
            _fail(f"{name}: FASTA input, standard input and bzip2 / xz / zstandard files need the text path (CUTSEQ_TEXT_PATH unset).")
    chunk_reads = switches.int_value("CHUNK_READS")
    if chunk_reads is None:
        chunk_reads = fastq.CHUNK_READS
    paired = tp.paired
    n_bins = len(tp.demux.barcodes) if tp.demux is not None else 0
    # the open file (or None) per [stream][mate]
    outs = [[fastq.OutputFile(n) if n else None for n in names] for names in args.outputs.name_groups(tp.swap_outputs)]
    too_long_route = args.outputs.too_long_route  # --too-long-output: stream 3 holds what -M catches
    # which (route, mate) streams go to disk, and whether they are gzip
    gz = [[(fh.gz if fh is not None else None) for fh in (group + [None])[:2]] for group in outs]

    totals = report.new_totals()
    progress = report.Progress()
    t0 = time.perf_counter()
    pool = fastq._pool()
    max_finishing = fastq.pool_size() + 2  # chunks being formatted / compressed (about 90 MB each)
    finishing: deque = deque()
    if tp.demux is not None:
        from . import demux  # look-up tables once, here: every device worker would otherwise build its own
        demux.ensure_tables(tp, devices[0])
    workers = [_DeviceWorker(tp, dev, chunk_reads) for dev in devices]

    def chunks():
        for k, chunk in enumerate(fastq.read_chunks(args.input_file[0], args.input_file[1] if paired else None,
                                                    chunk_reads, pinned=True)):
            if chunk.stride > abi.CS_MAX_STRIDE:
                record = k * chunk_reads + int(chunk.len1.argmax()) + 1
                chunk.release()
                raise ReadTooLong(f"reads longer than {abi.CS_MAX_STRIDE} nt are not supported by the GPU tile "
                                  f"(record {record} or its mate)")
            yield chunk

    def finish(chunk, r1, cap2, r2):
        """Pool job: records -> bytes on their way to disk; also this chunk's share of the report."""
        try:
            blobs, counts = fastq.finish_chunk(chunk, tp, r1, cap2, r2, gz, n_bins=n_bins, xflags=chunk.xflags,
                                               too_long_route=too_long_route)
            part = report.new_totals()
            report.account_chunk(part, tp, chunk.len1, r1, chunk.len2 if paired else None, r2 if paired else None,
                                 xflags=chunk.xflags)
            part["routes"] = counts[:3] if too_long_route else counts  # (its pairs are the totals' "too_long" already)
            return blobs, part
        finally:
            chunk.release()

    def emit(item):
        chunk, (r1, cap2, r2) = item
        progress.update(chunk.n)
        fut = pool.submit(finish, chunk, r1, cap2, r2)
        for route in range(len(outs)):
            for m in range(2 if paired else 1):
                if outs[route][m] is not None:
                    outs[route][m].write_job(fut, route, m)
        finishing.append(fut)
        while finishing and (len(finishing) >= max_finishing or finishing[0].done()):
            report.merge_totals(totals, finishing.popleft().result()[1])

    def merge_rest():
        first = None
        while finishing:  # every job is awaited: none may outlive the files it writes to
            try:
                report.merge_totals(totals, finishing.popleft().result()[1])
            except BaseException as exc:
                first = first or exc
        if first is not None:
            raise first

    fanout.run_ordered(workers, chunks(), emit, orphan=lambda item: item[0].release(), discard=lambda chunk: chunk.release(),
                       closers=[merge_rest] + [fh.close for group in outs for fh in group if fh is not None])
    # (after an error the pinned arena is left alone: parse / format jobs of the pool may still hold its buffers)
    fastq.PINNED.free_pinned()  # every chunk has been written and released
    stats = [w.stats for w in workers if w.stats is not None]
    totals["seconds"] = time.perf_counter() - t0
    progress.close()
    totals["bin_names"] = list(args.demux[0]) if n_bins else None
    totals["stats"] = stats
    if tp.has_poly_a:  # (--poly-a: PolyATrimmer.trimmed_bases per mate; a run without the option has no such key)
        totals["poly_a_bp"] = [sum(w.poly_a_bp[m] for w in workers if w.poly_a_bp is not None) for m in range(2)]
    totals["devices"] = devices
    return totals


def _refuse_bam_forms(args) -> None:
    """Unaligned BAM inputs (recognised by content) and what they do not combine with -- said before a device is touched.
    (Standard input is sniffed by its reader, once; it meets the same refusals there.)"""
    from . import codec
    kinds = {}
    for name in args.input_file:
        if name != "-" and os.path.isfile(name):
            container, first, _ = codec.sniff_input(name)
            kinds[name] = codec.is_bam(container, first)
    bams = [name for name, bam in kinds.items() if bam]
    if not bams:
        return
    if len(bams) < len(kinds):
        _fail("the two input files are in different formats (one BAM, one FASTQ or FASTA)")
    if args.ranks > 1 or args.rank_spec:
        _fail(f"{bams[0]}: only plain and gzip FASTQ files can be split between ranks")
    if not switches.enabled("TEXT_PATH"):
        _fail(f"{bams[0]}: BAM input needs the text path (CUTSEQ_TEXT_PATH unset): the record path is not extended to it.")


def run_cutseq(args, argv=None):
    barcode = BarcodeConfig(args.adapter_scheme)
    settings = settings_from_args(args)
    try:
        tp = compile_plan(args, barcode, settings)
    except ValueError as exc:  # e.g. a barcode list the demultiplexer cannot take: the CLI's exit style, no traceback
        _fail(str(exc))
    if settings.dry_run:
        dry_run(tp, barcode)
        return None
    # (standard input: the text path checks once it has seen the first byte)
    for option, wanted in (("--max-ee", tp.max_ee is not None), ("--nextseq-trim", tp.has_nextseq)):
        if wanted:
            from . import codec
            for name in args.input_file:
                if name != "-" and codec.sniff_input(name)[1][:1] in (b">", b"#"):
                    _fail(f"{option} needs qualities: {name} is a FASTA file.")
    _refuse_bam_forms(args)
    totals = None
    if args.rank_spec:  # a child of --ranks: its share, its part files, its totals; the parent reports
        from . import ranks
        spec = ranks.load_spec(args.rank_spec)
        args.outputs = args.outputs.with_rank_names(spec["outputs"])
        try:
            totals = run_pipeline(args, tp, shares=spec["inputs"])
        except (ValueError, OSError) as exc:
            from . import fastq
            # records out of step in THIS share (malformed record, mate ids that differ, unequal record counts): the one
            # failure that tells the parent its split by gzip members did not hold (ranks.RANK_EXIT_RECORDS)
            if isinstance(exc, fastq.FastqFormatError) or "IDs not identical" in str(exc) or "improperly paired" in str(exc):
                logging.error(str(exc))
                sys.exit(ranks.RANK_EXIT_RECORDS)
            raise
        ranks.dump_totals(spec, totals)
        return totals
    if args.ranks > 1:
        if not switches.enabled("TEXT_PATH"):
            logging.warning("--ranks ignored: it needs the text path.")
        else:
            from . import ranks
            totals = ranks.run_parent(list(sys.argv[1:] if argv is None else argv), args, tp)
    if totals is None:
        _phase("plan compiled")
        totals = run_pipeline(args, tp)
        _phase("pipeline done")
    if args.json_file:
        names, extra = args.outputs.report_names(args.input_file)
        report.write_json(args.json_file, report.json_report(tp, totals, barcode, *names, **extra))
    print(report.minimal_report(tp, totals), file=sys.stderr)
    return totals


def _block_records(args, n_devices: int) -> int:
    """Records per block of the text path: ``CUTSEQ_CHUNK_READS`` if set, else 262 144 -- less for small inputs, so
    that a short run does not allocate (and page-lock) for blocks it never fills: about two dozen blocks per device.
    (With the block buffers on huge pages the size matters little for a fresh 8 M-pair process -- 0.83 to 0.90 s for
    plain text with blocks of 65 536 to 262 144 records, and gzip input likes the big ones: 1.33 against 1.51 s;
    profiles/r03_cold_runs.log.)"""
    from . import textio
    fixed = switches.int_value("CHUNK_READS")
    if fixed is not None:
        return fixed
    try:
        size = os.path.getsize(args.input_file[0])
    except OSError:
        return textio.CHUNK_READS
    if args.input_file[0].endswith(".gz"):
        size *= 4  # (a guess at the text behind it)
    records = size // 300  # (a short-read record is ~330 bytes)
    if args.outputs.interleaved_in:  # (a block counts pairs, and this file holds both mates)
        records //= 2
    want = records // (24 * max(n_devices, 1))
    block = textio.CHUNK_READS
    while block > 16384 and block > want:
        block //= 2
    return block


def main(argv: Optional[List[str]] = None):
    _phase("main")
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0:
        parser.print_help(sys.stdout)
        sys.exit(0)
    args = resolve_args(parser.parse_args(argv))
    try:
        run_cutseq(args, argv)
    except (ReadTooLong, FileNotFoundError) as exc:  # user errors: the reference's exit style (run.py:1035-1039)
        _fail(str(exc))
    except RuntimeError as exc:
        if type(exc).__name__ != "RankFailure":
            raise
        _fail(f"{exc} -- its own message is above")  # (--ranks: the rank has already said what went wrong)


def console_main():
    """Entry point of the ``cutseq`` console script and of ``python -m cutseq_amd.run``.  When the run is over the
    process ends at once: unwinding the HIP runtime, its streams and gigabytes of page-locked memory takes longer than
    a short run itself (profiles/HISTORY.md), and the operating system reclaims all of it anyway.  Tools that
    collect their data when the process exits normally (rocprofv3 and friends preload a library) get the normal
    exit; so does anybody who sets CUTSEQ_FAST_EXIT=0."""
    traced = any("rocprof" in os.environ.get(k, "").lower() or "roctracer" in os.environ.get(k, "").lower()
                 for k in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB", "ROCPROFILER_REGISTER_FORCE_LOAD"))
    if traced or not switches.enabled("FAST_EXIT"):
        return main()
    code = 0
    try:
        main()
    except SystemExit as exc:
        code = exc.code if isinstance(exc.code, int) else (0 if exc.code is None else 1)
    except BaseException:
        import traceback
        traceback.print_exc()
        code = 1
    sys.stdout.flush()
    sys.stderr.flush()
    logging.shutdown()
    os._exit(code)


if __name__ == "__main__":
    console_main()
