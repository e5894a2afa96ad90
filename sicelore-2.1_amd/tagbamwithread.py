"""`tagbamwithread` (FJ!com/rw/tagbamwithread/TagWithReadSequenceMain.java:L85-116; sicelore-nf/main.nf:116): every BAM record that lies on
a reference gets its read's bases (and qualities) from the FASTQ as Z attributes.

    java -jar NanoporeBC_UMI_finder-2.1.jar tagbamwithread --inFastq <fastq[.gz]> --inBam <bam> --outBam <bam> --readTag US [--qvTag QS]

The FASTQ is inflated on the host (plain or multi-member gzip, as pigz writes it) and stays on the device as K-TAG's table of read names
(smi_tagbam_create); the BAM is read in segments of about segment_bytes compressed bytes (bamsegments.segments),
each segment's records tagged on the device (smi_tagbam_segment) and BGZF-deflated (on the device, or with zlib-level host threads) into
the output behind the input's header.  Records without a reference are dropped; a record whose read is not in the FASTQ is reported on
stderr and dropped, and the run goes on (L96-101).  No .bai is written (main.nf:117 runs `samtools index` right after) unless index=True
asks for the one htsjdk leaves beside the output (<outBam without .bam>.bai), built as the records are written (bamindex.WriterIndex)."""
import sys
import time

import numpy as np

from . import lib as _lib
from .bamsegments import BGZF_EOF, segments


def miss_message(name):
    """TagWithReadSequenceMain.java:L97-99, verbatim (two spaces after `for`)"""
    return f"ERROR: Did not find read for  SAM record, name: {name} Check whether fastq and BAM file correspond !"


def read_fastq_text(path, n_threads=4):
    """the FASTQ's text: gunzipped when the name ends in .gz (SplitFastqByChromosome.split L45-52), plain otherwise"""
    raw = np.fromfile(path, dtype=np.uint8)
    if path.endswith(".gz"):
        return _lib.gz_inflate(raw)
    return raw


def tag_bam_with_reads(ctx, in_fastq, in_bam, out_bam, read_tag, qv_tag=None, segment_bytes=256 << 20, n_threads=4, bgzf="device", hash_bits=0,
                       err=None, index=False):
    """`tagbamwithread -f in_fastq -b in_bam -o out_bam -r read_tag [-q qv_tag]` -> dict of counts (records in, written, unmapped dropped,
    missing) and seconds per phase.  The miss messages go to err (default sys.stderr) in record order.  bgzf: "device" (K-DEFLATE) or
    "zlib" (host threads, level 5).  hash_bits: test only (smi_tagbam_config).  index: also leave the .bai; the dict then has `index`
    (its counts and times; None when the records written are not in coordinate order: the BAM is kept and `index_error` says why)."""
    if bgzf not in ("device", "zlib"):
        raise ValueError("bgzf: 'device' or 'zlib'")
    err = sys.stderr if err is None else err
    t_all = time.perf_counter()
    secs = dict(fastq_read_inflate=0.0, fastq_table=0.0, bam_read_inflate=0.0, index=0.0, tag=0.0, bgzf_write=0.0)
    t0 = time.perf_counter()
    text = read_fastq_text(in_fastq, n_threads=n_threads)
    secs["fastq_read_inflate"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    table = _lib.TagBam(ctx, text, read_tag=read_tag, qv_tag=qv_tag, hash_bits=hash_bits)
    secs["fastq_table"] = time.perf_counter() - t0
    del text                                      # (the device holds its own copy)
    stage_ms = dict(key=0.0, build=0.0, probe=0.0, size=0.0, assemble=0.0)
    first = table.stage_ms()
    stage_ms["key"], stage_ms["build"] = first["key"], first["build"]

    n_in = n_written = n_unmapped = n_missing = 0
    stage = None
    wix, at = None, 0
    if index:
        from .bamindex import WriterIndex
        wix = WriterIndex(ctx)
    fh = open(out_bam, "wb")
    try:
        def emit(data, records=True):
            nonlocal at
            t1 = time.perf_counter()
            if data.size:
                if bgzf == "device":
                    z = ctx.bgzf_deflate_device(data)
                else:
                    z = _lib.bgzf_deflate(data, level=5, n_threads=n_threads)
                fh.write(memoryview(z[:-28]))       # without the end-of-file block: more follows
                if wix is not None:
                    wix.emitted(data, z[:-28], at, records)
                at += len(z) - 28
            secs["bgzf_write"] += time.perf_counter() - t1

        for bam, recs, hdr in segments(in_bam, segment_bytes, n_threads, secs):
            if hdr is not None:
                emit(np.frombuffer(hdr, dtype=np.uint8), records=False)  # the input's header bytes, as assignumis copies them (BamWriter L32-48)
            if recs.size:
                t1 = time.perf_counter()
                if stage is None or stage.array.size < 2 * bam.size:
                    if stage is not None:
                        stage.close()
                    stage = _lib.PinnedBuffer(int(2.2 * bam.size) + (1 << 20))
                out, missing, unmapped = table.segment(bam, recs, out=stage.array)
                ms = table.stage_ms()
                for k in ("probe", "size", "assemble"):
                    stage_ms[k] += ms[k]
                if missing.size:
                    err.write("".join(miss_message(_lib_read_name(bam, recs[int(i)])) + "\n" for i in missing))
                    err.flush()
                n_in += int(recs.size)
                n_missing += int(missing.size)
                n_unmapped += int(unmapped)
                n_written += int(recs.size) - int(missing.size) - int(unmapped)
                secs["tag"] += time.perf_counter() - t1
                emit(out)
        fh.write(BGZF_EOF)
        fh.close()
        extra = {}
        if wix is not None:
            bai = (out_bam[:-4] if out_bam.endswith(".bam") else out_bam) + ".bai"      # htsjdk's name for it
            extra["index"], extra["index_error"] = wix.finish(bai, at, log=err)
    finally:
        fh.close()
        table.close()
        if wix is not None:
            wix.close()
        if stage is not None:
            stage.close()
    return dict(records=n_in, written=n_written, unmapped=n_unmapped, missing=n_missing, fastq_records=table.n_records, seconds=secs,
                stage_ms=stage_ms, wall_s=time.perf_counter() - t_all, **extra)


def _lib_read_name(bam, rec):
    o, n = int(rec["name_off"]), max(int(rec["l_read_name"]) - 1, 0)
    return bam[o:o + n].tobytes().decode("latin-1")

