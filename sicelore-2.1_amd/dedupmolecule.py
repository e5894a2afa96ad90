"""`DeduplicateMolecule` (org/ipmc/sicelore/programs/DeduplicateMolecule.java:L41-302; the reference README's step 4b, sicelore-nf/main.nf:184):
one record per molecule out of the concatenated per-chromosome consensus files.

    java -jar Sicelore-2.1.jar DeduplicateMolecule -I molecules.fastq -O deduplicate.fastq -SELECT true -VALIDATION_STRINGENCY SILENT

A streaming filter in two passes over the input, read in segments of about segment_bytes: pass 1 (smi_dedup_add_segment) finds the records
of a segment, parses their names and keeps key, rn and lengths on the device; what a segment leaves unconsumed (the record its end cuts) is
read again in front of the next one.  smi_dedup_select builds the molecule table and picks each molecule's record; pass 2
(smi_dedup_emit_segment) reads the same segments again and writes the winners, in input order.  The output file is
created only when pass 1 and the selection succeeded."""
import os
import time

import numpy as np

from . import lib as _lib


def is_fastq(path):
    """L46: the file name, lower-cased, ends in .fq or .fastq; everything else is read as single-line FASTA"""
    name = os.path.basename(path).lower()
    return name.endswith(".fq") or name.endswith(".fastq")


def reference_log(info, fasta, select):
    """the reference's log lines (L110, L145-151, L171; L182, L225-231, L251; L262, L298-301) without htsjdk's prefix"""
    c, m = info["records"], info["molecules"]
    if fasta:
        return ["loadFasta\tSTART...", "loadFasta\tEND...", f"loadFasta\t{c} sequences loaded", "loadFasta tso\t0", f"loadFasta\t{m} molecules",
                "loadFasta\tEND...", "writeFasta\tSTART...", "writeFasta\tEND..."]
    if select:
        return ["loadFastQ\tSTART...", "loadFastQ\tEND...", f"loadFastQ\t{c} sequences loaded", "loadFastQ tso\t0", f"loadFastQ\t{m} molecules",
                "loadFastQ\tEND...", "writeFastQ\tSTART...", "writeFastQ\tEND..."]
    return ["load/write FastQ\tSTART...", "load/write FastQ\tEND...", f"loadFastQ\t{c} sequences loaded", "loadFastQ tso\t0",
            f"loadFastQ\t{m} molecules"]


def _read(f, pos, n):
    f.seek(pos)
    return np.frombuffer(f.read(n), dtype=np.uint8)


def deduplicate_molecule(ctx, in_path, out_path, select=True, segment_bytes=256 << 20, log=None, **knobs):
    """-> dict of the counters (lines, records = the reference's count, null_records, skipped_lines, molecules, bytes_written, segments,
    table_slots, probe_steps, wraps), `reads` = (file offset, bytes read, bytes consumed) per segment, device ms per stage and seconds.
    knobs: hash_bits, min_table_slots (smi_dedup_config).  log: a text stream for the reference's log lines."""
    t_all = time.perf_counter()
    if in_path.lower().endswith(".gz"):
        raise _lib.SmiError(f"DeduplicateMolecule: I={in_path}: a .gz input is not read (the reference would take its compressed bytes for FASTA): "
                            "decompress it first")
    if segment_bytes < 1:
        raise ValueError("segment_bytes must be at least 1")
    fasta = not is_fastq(in_path)
    h = _lib.Dedup(ctx, fasta=fasta, select=select, **knobs)
    reads = []
    try:
        with open(in_path, "rb") as f:
            size = os.fstat(f.fileno()).st_size
            t0 = time.perf_counter()
            pos, want = 0, segment_bytes
            while True:
                buf = _read(f, pos, want)
                last = pos + buf.size >= size
                used = h.add_segment(buf, last)
                if used == 0 and not last:       # one record (or line) longer than the segment
                    want *= 2
                    continue
                reads.append((pos, int(buf.size), used))
                pos += used
                want = segment_bytes
                if last:
                    break
            h.select()
            t_pass1 = time.perf_counter() - t0
            t0 = time.perf_counter()
            written = 0
            with open(out_path, "wb") as out:
                for k, (at, _n, used) in enumerate(reads):
                    part = h.emit_segment(k, _read(f, at, used))
                    out.write(part)
                    written += len(part)
            t_pass2 = time.perf_counter() - t0
        counts = h.counts()
        stage_ms = h.stage_ms()
    finally:
        h.close()
    laid_out = counts.pop("bytes_out")
    if written != laid_out:
        raise _lib.SmiError(f"DeduplicateMolecule: {written} bytes written, {laid_out} laid out")
    info = dict(counts, bytes_written=written, reads=reads, stage_ms=stage_ms, seconds=dict(pass1=t_pass1, pass2=t_pass2),
                wall_s=time.perf_counter() - t_all)
    if log is not None:
        for line in reference_log(info, fasta, select):
            print(line, file=log)
    return info
