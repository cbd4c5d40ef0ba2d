"""cutadapt's --interleaved as a rule on text: pairs in one stream, the record of one mate, then the record of the other.

The expected value of every interleaved run is this rule applied to the two-file run of the same records: an
interleaved input is ``weave`` of the two input texts, an interleaved output is ``weave`` of the two output streams.
Nothing here knows the engine."""


def _records(text: bytes, lines_per_record: int):
    """The records of ``text``, every line with the line end it came with ('\\n', '\\r\\n', or none on the last line)."""
    lines = text.splitlines(keepends=True)
    if len(lines) % lines_per_record:
        raise ValueError(f"{len(lines)} lines are no whole number of {lines_per_record}-line records")
    return [b"".join(lines[i:i + lines_per_record]) for i in range(0, len(lines), lines_per_record)]


def deinterleave(text: bytes):
    """Interleaved FASTQ -> (text of mate 1, text of mate 2), by four-line records: records 0, 2, 4, ... are mate 1's.
    Line ends are kept as they are; the last line may lack its own."""
    recs = _records(text, 4)
    if len(recs) % 2:
        raise ValueError("an odd number of records: the last one has no partner")
    return b"".join(recs[0::2]), b"".join(recs[1::2])


def weave(stream1: bytes, stream2: bytes, fasta: bool = False, mate2_first: bool = False) -> bytes:
    """The interleaved stream of two mate streams: records alternate, four lines each (two for FASTA), mate 1's first
    unless ``mate2_first``.  A record that lacked its last line end and does not end the woven stream gets '\\n'."""
    per = 2 if fasta else 4
    a, b = _records(stream1, per), _records(stream2, per)
    if len(a) != len(b):
        raise ValueError(f"{len(a)} records of mate 1 and {len(b)} of mate 2")
    if mate2_first:
        a, b = b, a
    out = [rec for pair in zip(a, b) for rec in pair]
    for i, rec in enumerate(out[:-1]):
        if not rec.endswith(b"\n"):
            out[i] = rec + b"\n"
    return b"".join(out)
