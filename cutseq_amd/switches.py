"""Every ``CUTSEQ_*`` environment variable the product knows, and the one place where the Python layer reads them.

``TABLE`` is the list: the switches read here, and those the native library reads itself (``getenv`` in
``csrc/cutseq_hip.hip``: when a plan, an engine or a text engine is created, per object; the huge-page answer once per
process).  A caller names a switch by its entry -- ``switches.enabled("TEXT_PATH")`` -- and gets the parsed value;
spelling, default and parse live here.  Nothing is cached: a switch is sampled when the accessor is called, and the
callers decide when that is (``INTEGRATION.md`` section 4 has the list for users).

The two layers parse flags differently and stay that way: here a default-on flag is off at exactly ``"0"`` and a
default-off flag is on at exactly ``"1"``; the library goes by ``atoi``, so ``"00"`` is off there and on here.
"""
from __future__ import annotations

import os
from typing import List, NamedTuple, Optional

FLAG_ON, FLAG_OFF, INT, DEVICES, PATH = "flag, default on", "flag, default off", "int", "device list", "path"
PREFIX = "CUTSEQ_"


class Switch(NamedTuple):
    name: str      # the variable; callers say it without the prefix
    kind: str
    default: object
    reader: str    # "python", "native" or "both"
    meaning: str


TABLE = (
    # path switches: the tests hold both settings to equal output
    Switch("CUTSEQ_TEXT_PATH", FLAG_ON, True, "python", "0: the record path (host parser and formatter) instead of the text path"),
    Switch("CUTSEQ_GPU_DEFLATE", FLAG_ON, True, "python", "0: gzip outputs are deflated in the host pool, not on the device"),
    Switch("CUTSEQ_GPU_LZ", FLAG_ON, True, "native", "0: the device's gzip members without their LZ77 stage"),
    Switch("CUTSEQ_GPU_INFLATE", FLAG_OFF, False, "python", "1: BGZF FASTQ input is inflated on the device and its text stays there (one GPU, no --ranks)"),
    Switch("CUTSEQ_OWN_INFLATE", FLAG_ON, True, "python", "0: libdeflate inflates gzip input, not the package's decoder"),
    Switch("CUTSEQ_PARALLEL_INFLATE", FLAG_ON, True, "python", "0: single-member gzip input is inflated serially"),
    Switch("CUTSEQ_PAIR", FLAG_ON, True, "native", "0: the chain's leading 5' + 3' ops as two scans, not one merged walk"),
    Switch("CUTSEQ_EXISTS", FLAG_ON, True, "native", "0: the exact filter for the 5' op, not the existence-only scan"),
    Switch("CUTSEQ_CUT_RUNS", FLAG_ON, True, "native", "0: one op-loop turn per CUT op"),
    Switch("CUTSEQ_ITEM_SLOTS", INT, None, "native", "1..16: slots per lane in the leading walk's item log (default: what fits)"),
    Switch("CUTSEQ_FAST_RECODE", INT, 1, "native", "0: exact re-coding of every tile; 2 (tests only): no fallback, mis-codes reads outside ACGTN"),
    Switch("CUTSEQ_PINNED_THP", FLAG_ON, True, "both", "0: page-locked buffers from hipHostMalloc, not from transparent huge pages"),
    Switch("CUTSEQ_DEVICES", DEVICES, None, "python", "GPUs to use, one entry per rank or worker, repeats allowed (default: all)"),
    Switch("CUTSEQ_CHUNK_READS", INT, None, "python", "records per block (default: sized to the input)"),
    Switch("CUTSEQ_HOST_THREADS", INT, None, "native", "bound of the library's host threads; fastq.set_threads writes it (-t/--threads)"),
    Switch("CUTSEQ_HIP_LIB", PATH, None, "python", "the trimming library to load instead of the package's own (A/B builds)"),
    # diagnostics
    Switch("CUTSEQ_PROGRESS", FLAG_ON, True, "python", "0: no progress line and no Done line"),
    Switch("CUTSEQ_PROFILE", FLAG_OFF, False, "python", "1: seconds per phase, thread and activity on standard error"),
    Switch("CUTSEQ_DISCARD_OUTPUT", FLAG_OFF, False, "python", "1: the writers drop their bytes"),
    Switch("CUTSEQ_DEBUG_INFLATE", FLAG_OFF, False, "python", "1: which chunk of the parallel inflate lost its proof, and how"),
    Switch("CUTSEQ_FAST_EXIT", FLAG_ON, True, "python", "0: the console script unwinds the runtime instead of exiting at once"),
    # tests only
    Switch("CUTSEQ_LOG_ALWAYS", FLAG_OFF, False, "native", "1: every adapter op counts as log-friendly (short adapters through the merged walk)"),
    # leftovers of the hand-out and grid sweeps (cs_engine_create): no test, tool or document uses them; to be deleted
    Switch("CUTSEQ_COL_BYTES", INT, None, "native", "1024..32768: LDS bytes of DP scratch per resolve wave, if more than the plan needs"),
    Switch("CUTSEQ_BATCH_KNOB", INT, 1, "native", "resolve kernel: scales the record counts below which batches shrink to 32 / 16 records"),
    Switch("CUTSEQ_RESOLVE_WAVES", INT, 4, "native", "1..16: resolve waves per CU in pipelined calls"),
    Switch("CUTSEQ_GRID_X", INT, None, "native", "blocks of the scan kernel's grid (default: twice the resident set)"),
    Switch("CUTSEQ_UNITS", INT, None, "native", "three numbers \"big_shift,small_shift,big_pct\": the scan kernel's tile hand-out units"),
)
_BY_KEY = {s.name[len(PREFIX):]: s for s in TABLE}


def _lookup(key: str, *kinds: str) -> Switch:
    s = _BY_KEY[key]
    if s.kind not in kinds or s.reader == "native":
        raise TypeError(f"{s.name} is a {s.kind} switch read by: {s.reader}")
    return s


def enabled(key: str) -> bool:
    """A flag of either kind: the table's default unless the variable holds the one string that flips it."""
    s = _lookup(key, FLAG_ON, FLAG_OFF)
    value = os.environ.get(s.name)
    return value != "0" if s.kind == FLAG_ON else value == "1"


def int_value(key: str) -> Optional[int]:
    """The number, or the table's default when the variable is unset or empty; anything else raises ValueError."""
    s = _lookup(key, INT)
    value = os.environ.get(s.name)
    return int(value) if value else s.default


def device_list(key: str, n_default: int) -> List[int]:
    """``"0,0,1"`` -> [0, 0, 1]; unset or empty: the first ``n_default`` devices.  Range checks are the caller's."""
    s = _lookup(key, DEVICES)
    value = os.environ.get(s.name)
    return [int(x) for x in value.split(",")] if value else list(range(n_default))


def path(key: str, default: str) -> str:
    s = _lookup(key, PATH)
    return os.environ.get(s.name, default)
