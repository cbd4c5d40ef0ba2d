"""Which output files a run writes, decided once.

``resolve`` (called by ``run.resolve_args``) turns the command line into one :class:`OutputLayout`, kept as
``args.outputs``: the output classes of the run, the file (if any) that receives each class per mate, and whether the
mates share a file.  The pipelines, the ranks and the JSON report read it; nobody derives any of it again.
:class:`TextOptions` is what a text engine has to know of it (``textio.text_options`` builds one).
"""
from __future__ import annotations

import dataclasses
import logging
import sys
from dataclasses import dataclass
from typing import List, Optional, Tuple

from .common import remove_fq_suffix

# Output naming (user-visible contract of the reference CLI, run.py:1058-1107): for every output class the
# files are, in this order of precedence, the ones given on the command line (one per input file), the
# -O prefix, or the input name without its FASTQ suffix, followed by "_<class>_R<mate>.fastq.gz".
OUTPUT_CLASSES = (  # (argparse attribute, word in the file name)
    ("output_file", "trimmed"),
    ("short_file", "short"),
    ("untrimmed_file", "untrimmed"),
)
TOO_LONG_CLASS = ("too_long_file", "too-long")  # --too-long-output: the given names or none, no default from -O


def _fail(message: str):
    logging.error(message)
    sys.exit(1)


def output_paths(given, inputs, prefix, word, interleaved=None):
    """File names of one output class, one per input file.  ``interleaved`` (an ``--interleaved`` run): "out" -- the
    class is ONE file of interleaved pairs, ``<stem>_<word>.fastq.gz`` --, or "split" -- one interleaved input file,
    two output files; the stem comes from ``-O`` or from the first input file."""
    if interleaved:
        want = 1 if interleaved == "out" else 2
        if given:
            if len(given) != want:
                _fail(f"Number of {word} output files ({len(given)}) must match the number this --interleaved run "
                      f"writes per class: {want} ({'interleaved' if want == 1 else 'one per mate'}).")
            return list(given)
        stem = prefix if prefix is not None else remove_fq_suffix(inputs[0])
        return [f"{stem}_{word}.fastq.gz"] if want == 1 else [f"{stem}_{word}_R{mate}.fastq.gz" for mate in (1, 2)]
    if given:
        if len(given) != len(inputs):
            _fail(f"Number of {word} output files ({len(given)}) must match number of input files ({len(inputs)}).")
        return list(given)
    stems = [prefix] * len(inputs) if prefix is not None else [remove_fq_suffix(name) for name in inputs]
    return [f"{stem}_{word}_R{mate}.fastq.gz" for mate, stem in enumerate(stems, 1)]


@dataclass(frozen=True)
class OutputClass:
    key: str                          # the argparse attribute; a barcode's class: the barcode's name
    word: str                         # the word in default file names
    route: int                        # the device's route class: 0 trimmed, 1 too short, 2 untrimmed, 3 too long / barcodes
    names: Tuple[Optional[str], ...]  # the file per mate (one entry where the mates share a file); None: no such file
    barcode: bool = False


@dataclass(frozen=True)
class OutputLayout:
    """``classes``: trimmed, too short, untrimmed, then either too long (``--too-long-output``) or one class per
    barcode (``--demux-barcodes``), never both.  A demultiplexing run keeps the common trimmed names for its report
    and writes nothing under them."""
    paired: bool
    classes: Tuple[OutputClass, ...]
    interleaved_in: bool = False      # --interleaved: one input file holds both mates
    interleaved_out: bool = False     # ... every class is one file of woven pairs
    info_file: Optional[str] = None
    bgzf: bool = False                # --bgzf: every output whose container is gzip is written as BGZF

    @classmethod
    def of(cls, trimmed, short, untrimmed, too_long=None, barcodes=None, **flags) -> "OutputLayout":
        """From the names per class (``barcodes``: {barcode name: its trimmed files})."""
        classes = [OutputClass(key, word, route, tuple(names))
                   for route, ((key, word), names) in enumerate(zip(OUTPUT_CLASSES, (trimmed, short, untrimmed)))]
        if too_long:
            classes.append(OutputClass(*TOO_LONG_CLASS, 3, tuple(too_long)))
        for name, names in (barcodes or {}).items():
            classes.append(OutputClass(name, f"{name}_trimmed", 3, tuple(names), barcode=True))
        return cls(classes=tuple(classes), **flags)

    @property
    def n_bins(self) -> int:
        return sum(c.barcode for c in self.classes)

    @property
    def too_long_route(self) -> bool:
        """--too-long-output: what -M catches is route 3, a fourth stream."""
        return any(c.route == 3 and not c.barcode for c in self.classes)

    @property
    def untrimmed_requested(self) -> bool:
        return all(name is not None for name in self.classes[2].names)

    def name_groups(self, swap_outputs: bool) -> List[list]:
        """The output files' names by the stream they receive -- [trimmed, too short, untrimmed, barcode 0, barcode 1,
        ...] or [trimmed, too short, untrimmed, too long] --, one entry per mate each (None: no such file).  Paired
        --auto-rc on a '-' library (``swap_outputs``) swaps the mates' trimmed files (cutseq/run.py:787-791), the
        barcodes' too and no others.  An interleaved output has one name per class and nothing to swap: the device
        writes mate 2's record first instead (``mate2_first``)."""
        swap = self.paired and swap_outputs and not self.interleaved_out
        groups = []
        for c in self.classes:
            names = [None] * len(c.names) if c.route == 0 and self.n_bins else list(c.names)
            groups.append(names[::-1] if swap and (c.route == 0 or c.barcode) else names)
        return groups

    def names(self, info: bool = True) -> List[str]:
        """Every file this run writes (``info``: the --info-file table among them)."""
        return [n for group in self.name_groups(False) for n in group if n] + ([self.info_file] if info and self.info_file else [])

    def _rank_keys(self):
        bins = iter(range(self.n_bins))
        return [(f"demux_files:{next(bins)}" if c.barcode else c.key, c) for c in self.classes]

    def rank_groups(self) -> dict:
        """{key of a rank's spec: the output files under it}: every rank writes a part of each and the parts are
        concatenated in rank order."""
        groups = {key: group for (key, _), group in zip(self._rank_keys(), self.name_groups(False))}
        if self.info_file:  # every rank's table of its share; concatenated in rank order like the records
            groups["info_file"] = [self.info_file]
        return groups

    def with_rank_names(self, mapping: dict) -> "OutputLayout":
        """The layout of one rank: the names of ``mapping`` (a rank spec's ``rank_groups``) in place of the run's."""
        classes = tuple(dataclasses.replace(c, names=tuple(mapping[key])) if key in mapping else c for key, c in self._rank_keys())
        return dataclasses.replace(self, classes=classes, info_file=mapping.get("info_file", [self.info_file])[0])

    def report_names(self, inputs):
        """-> (positional, keyword) arguments of ``report.json_report`` behind the barcode.  The mate-2 keys are null
        where one file holds both mates: interleaved input, interleaved output."""
        too_long = [list(c.names) for c in self.classes if c.route == 3 and not c.barcode]
        return (self._both(inputs) + [n for c in self.classes[:3] for n in self._both(c.names)],
                dict(info_file=self.info_file, too_long_files=too_long[0] if too_long else None, interleaved=self.interleaved_in))

    def _both(self, names) -> list:
        return [names[0], names[1] if self.paired and len(names) > 1 else None]


def resolve(args, interleaved_in: bool, interleaved_out: bool, wants_untrimmed: bool) -> OutputLayout:
    """The layout of a validated command line (``args.demux``: the barcode list read, or None)."""
    inputs = args.input_file
    form = "out" if interleaved_out else ("split" if interleaved_in else None)
    too_long = output_paths(args.too_long_file, inputs, None, TOO_LONG_CLASS[1], form) if args.too_long_file else None
    three = [output_paths(vars(args)[attr], inputs, args.output_prefix, word, form)
             if attr != "untrimmed_file" or wants_untrimmed else [None] * ({"out": 1, "split": 2}.get(form) or len(inputs))
             for attr, word in OUTPUT_CLASSES]
    barcodes = None
    if args.demux is not None:  # one pair of trimmed files per barcode instead of the common one
        barcodes = {name: output_paths(None, inputs, args.output_prefix, f"{name}_trimmed") for name in args.demux[0]}
    return OutputLayout.of(*three, too_long, barcodes, paired=len(inputs) == 2 or interleaved_in or interleaved_out,
                           interleaved_in=interleaved_in, interleaved_out=interleaved_out, info_file=args.info_file,
                           bgzf=bool(getattr(args, "bgzf", False)))


@dataclass(frozen=True)
class TextOptions:
    """What a text engine is told about the outputs (the keywords of ``textpath.TextEngine`` of the same names)."""
    compress: int = False         # every route leaves the device as a gzip member (True) or as BGZF blocks (2: --bgzf)
    bins: int = 0                 # demultiplexing: one route per barcode behind the three ordinary ones
    fasta_routes: int = 0         # bit 2 * class + mate: that stream's records leave as FASTA
    info: int = 0                 # abi.CS_INFO_* bits: the batches also yield the --info-file table
    too_long_route: bool = False  # --too-long-output: the pairs -M catches are a fourth stream (route 3)
    interleave_in: bool = False   # --interleaved: an item is (block of both mates, None) ...
    interleave_out: bool = False  # ... the routes come back as one stream each
    mate2_first: bool = False
