"""Per-file output format, the parts that need no GPU: ``textio.output_formats`` (dnaio's rule file by file ->
``cs_text_params.fasta_routes``) and the field's place in the ABI.

Reference: ``OutputFiles.open_record_writer`` hands every name to dnaio on its own (cutseq/run.py:437-441, 449, 465,
754-758), so FASTA and FASTQ files in one run are valid there."""
import ctypes as C
import itertools
import re
from pathlib import Path

import pytest

from cutseq_amd import abi, fastq, ranks, textio
from cutseq_amd.outputs import OutputLayout

ROOT = Path(__file__).resolve().parent.parent

# name -> what the name itself says (None: nothing, the input decides)
NAMES = {"a.fastq.gz": "fastq", "a.fq": "fastq", "a.fa": "fasta", "a.fasta.xz": "fasta", "a.txt": None, "-": None,
         None: "absent"}


def want_mask(groups, has_qualities):
    """The rule of the docstring of ``textio.output_formats``, restated: per file its extension, else the input;
    a stream without a file follows the input unless every file there is is FASTA.

    The per-file part is dnaio's rule and is what this function checks.  The part about streams WITHOUT a file is the
    project's own choice (their bytes are dropped, so no reference says what they should be); restating it here only
    pins it, it does not prove it."""
    follow = "fastq" if has_qualities else "fasta"
    kinds = [[(NAMES[n] or follow) if n else None for n in g] for g in groups]
    named = {k for g in kinds for k in g if k}
    absent = "fasta" if named == {"fasta"} else follow
    mask = 0
    for q, g in enumerate(kinds):
        for m, k in enumerate(g):
            if (k or absent) == "fasta":
                mask |= 1 << (2 * min(q, 3) + m)
    return mask


@pytest.mark.parametrize("has_qualities", [True, False])
def test_every_combination_of_names_single_end(has_qualities):
    """7 choices for each of trimmed / short / untrimmed / the barcodes' files (two barcodes, one template)."""
    seen = set()
    for t, s, u, b in itertools.product(NAMES, repeat=4):
        groups = [[t], [s], [u]] + ([[b], [b]] if b else [])
        fastq_named = [n for g in groups for n in g if n and NAMES[n] == "fastq"]
        if fastq_named and not has_qualities:
            with pytest.raises(fastq.FastqFormatError) as exc:
                textio.output_formats(groups, has_qualities)
            assert "Output format cannot be FASTQ since no quality values are available" in str(exc.value)
            assert repr(fastq_named[0]) in str(exc.value)
            continue
        got = textio.output_formats(groups, has_qualities)
        assert got == want_mask(groups, has_qualities), (groups, has_qualities)
        assert got & 0xAA == 0 and (b or got & 0xC0 == 0)  # no bit of a stream that does not exist
        seen.add(got)
    assert len(seen) > (8 if has_qualities else 1)  # (FASTA input: every stream FASTA, with and without bins)


@pytest.mark.parametrize("has_qualities", [True, False])
def test_every_combination_of_names_paired(has_qualities):
    """The mates of a class vary on their own: 7 x 7 names per class, the classes two at a time against fixed others."""
    pairs = list(itertools.product(NAMES, repeat=2))
    fixed = [["a.fq", "a.fa"], [None, None], ["-", "a.fasta.xz"]]
    for cls in range(4):
        for a, b in pairs:
            groups = [list(g) for g in fixed]
            if cls < 3:
                groups[cls] = [a, b]
            elif a or b:
                groups += [[a, b], [a, b], [a, b]]
            named = [n for g in groups for n in g if n]
            if not has_qualities and any(NAMES[n] == "fastq" for n in named):
                with pytest.raises(fastq.FastqFormatError):
                    textio.output_formats(groups, has_qualities)
                continue
            assert textio.output_formats(groups, has_qualities) == want_mask(groups, has_qualities), (groups, has_qualities)
    # spelled out once: trimmed R1 FASTQ / R2 FASTA, short files both FASTA, no untrimmed files (they follow the input)
    assert textio.output_formats([["t1.fastq.gz", "t2.fa.gz"], ["s1.fa", "s2.fasta"], [None, None]], True) == 0b001110
    assert textio.output_formats([["t1.fa", "t2.fa"], [None, None], [None, None]], True) == 0b111111  # one format: all of it
    assert textio.output_formats([["t1.fq", "t2.fq"], [None, None], [None, None]], True) == 0
    assert textio.output_formats([[None, None]] * 3 + [["b_R1.fa", "b_R2.fq"]] * 4, True) == 0b01000000
    assert textio.output_formats([[None, None], ["s1.fa", "s2.fa"], [None, None], [None, None]], True) == 0xFF


def test_bins_of_a_mate_share_one_format():
    with pytest.raises(ValueError, match="all bins of a mate share one format"):
        textio.output_formats([[None], [None], [None], ["a.fa"], ["b.fq"]], True)


def test_format_goes_with_the_file_not_with_the_mate():
    """Paired --auto-rc on a '-' library: mate 1's trimmed records are written to the SECOND -o file
    (textio.run_text_pipeline swaps the trimmed pair and the barcodes' pairs).  The groups are handed over after the
    swap, so the bit of mate 0 comes from the second name."""
    out = ["t_R1.fastq", "t_R2.fasta"]
    assert textio.output_formats([out, [None, None], [None, None]], True) == 0b10
    assert textio.output_formats([out[::-1], [None, None], [None, None]], True) == 0b01


def test_run_text_pipeline_swaps_before_it_asks(monkeypatch, tmp_path):
    """... and the pipeline does hand them over swapped: caught at the call, before any device is touched."""
    import argparse
    import gzip

    seen = {}

    class Stop(Exception):
        pass

    def spy(groups, has_qualities):
        seen["groups"], seen["q"] = [list(g) for g in groups], has_qualities
        raise Stop

    monkeypatch.setattr(textio, "output_formats", spy)
    ins = []
    for m in (1, 2):
        p = tmp_path / f"in{m}.fq.gz"
        with gzip.open(p, "wb") as fh:
            fh.write(b"@r/%d\nACGT\n+\nIIII\n" % m)
        ins.append(str(p))

    class Plan:
        paired, demux = True, None

    for swap in (False, True):
        Plan.swap_outputs = swap
        args = argparse.Namespace(input_file=ins, outputs=OutputLayout.of(["t1.fq", "t2.fa"], ["s1.fa", "s2.fq"], [None, None],
                                                                          paired=True))
        with pytest.raises(Stop):
            textio.run_text_pipeline(args, Plan, [0], 1000)
        assert seen["q"] is True
        assert seen["groups"] == [["t2.fa", "t1.fq"] if swap else ["t1.fq", "t2.fa"], ["s1.fa", "s2.fq"], [None, None]]

    # a demultiplexing plan handed over without files for its barcodes: their (dropped) streams are asked about all the
    # same, as one class-3 group without names, so that they take the format of everything else
    class Demux:
        barcodes = ["ACGT", "TGCA"]

    Plan.demux, Plan.swap_outputs = Demux, False
    args = argparse.Namespace(input_file=ins, outputs=OutputLayout.of([None, None], ["s1.fa", "s2.fa"], [None, None],
                                                                      barcodes={"": [None, None]}, paired=True))
    with pytest.raises(Stop):
        textio.run_text_pipeline(args, Plan, [0], 1000)
    assert seen["groups"] == [[None, None], ["s1.fa", "s2.fa"], [None, None], [None, None]]


def test_output_format_keeps_its_rule():
    """The one-format function stays what tests/test_host_io.py pins, mixed names refused included."""
    with pytest.raises(ValueError, match="one format per run"):
        textio.output_format(["a.fasta", "b.fastq"], True)
    assert textio.output_format(["a.fasta", "b.fa.gz"], True) is True
    assert textio.output_format(["a.txt"], True) is False


def test_abi_field():
    assert abi.CS_ABI_VERSION == 7
    assert C.sizeof(abi.cs_text_params) == 48
    f = abi.cs_text_params.fasta_routes
    assert f.size == 1 and f.offset == abi.cs_text_params.fasta_out.offset + 1 == 45
    p = abi.cs_text_params()
    assert p.fasta_routes == 0  # a caller that never heard of it: fasta_out alone decides
    # the header agrees: the same members in the same order, so the same offsets (all of them naturally aligned)
    header = (ROOT / "include" / "cutseq_hip.h").read_text()
    body = re.search(r"typedef struct cs_text_params \{(.*?)\} cs_text_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [(m.group(1).strip(), m.group(2), m.group(3)) for m in
               re.finditer(r"([A-Za-z_0-9 ]+?[ \*]+)([a-z_0-9]+)(\[\d+\])?;", body)]
    size = {"uint8_t": 1, "uint32_t": 4, "const char *": 8}
    at, offsets = 0, {}
    for ctype, name, dim in members:
        width = size[ctype.strip() if "*" not in ctype else "const char *"]
        at = (at + width - 1) // width * width
        offsets[name] = at
        at += width * (int(dim[1:-1]) if dim else 1)
    assert (at + 7) // 8 * 8 == 48
    assert [name for _c, name, _d in members] == [name for name, _t in abi.cs_text_params._fields_]
    for name, _t in abi.cs_text_params._fields_:
        assert offsets[name] == getattr(abi.cs_text_params, name).offset, name


def test_rank_parts_keep_the_format_of_their_file():
    """--ranks: every rank but the first writes a part file beside the final one.  Its records go by ITS name, so the
    part's name must say what the file's says."""
    for final in ("t1.fastq.gz", "t2.fa.gz", "s1.FA", "s2.fq", "u.txt", "x.fasta.xz", "y.fna.zst", "plain"):
        assert ranks.part_name(final, 0) == final
        part = ranks.part_name(final, 1)
        assert part != final and part.startswith(final) and part != ranks.part_name(final, 2)
        assert textio.format_of_name(part) == textio.format_of_name(final), (part, final)
        for ending in (".gz", ".bz2", ".xz", ".zst"):
            assert part.endswith(ending) == final.endswith(ending)
    assert ranks.part_name(None, 1) is None
