"""`FusionDetector` (org/ipmc/sicelore/programs/FusionDetector.java:L54-113; the reference README's step 6, "Fusion transcripts detection
cell by cell"): the molecules of a tagged BAM (BC / U8 / GE, optional RN, de / df) whose reads name exactly two genes, counted per cell.

    java -jar Sicelore-2.1.jar FusionDetector I=clipped_reads.tags.US.bam O=. PREFIX=fusion CSV=ValidBarcodes.csv

The BAM is read once in segments of about segment_bytes compressed bytes, inflated one segment ahead by a reader thread
(bamsegments.segments) and filtered by the library's host threads (smi_fusion_add_segment); reads, molecules and gene names are grouped
by their bytes on the device and K-MTX renders the matrix (smi_fusion_run).  Cells and rows are in byte order, molinfos in (cell, UMI) byte
order.  A record the parser fails on stops the run before any file is written."""
import os
import time

from . import lib as _lib
from .bamsegments import segments


def fusions_of(metrics):
    """the (key, molecules) rows of a PREFIX_fusmetrics.txt text (bytes): `key \\t key \\t na \\t total`"""
    out = []
    for line in metrics.split(b"\n")[1:]:
        if not line:
            continue
        head, _sep, total = line.rpartition(b"\tna\t")
        out.append((head[:(len(head) - 1) // 2].decode("latin-1"), int(total)))
    return out


def statistics_lines(c, fusions):
    """the messages of the reference's run in order (FusionDetector.java:L60, L70, L103; LongreadParser.java:L51, L84-93;
    MoleculeDataset.java:L63, L85, L96-97), without the logger's prefix.  fusions: (key, molecules) pairs; a key with 10 molecules or more
    is named, by molecules descending, ties in byte order of the key."""
    lines = [
        f"\tCells detected\t[{c['cells']}]",
        "\tstart...",
        "\tend...",
        f"\tTotal SAMrecords\t{c['records']}",
        f"\tSAMrecords valid\t{c['valid']}",
        f"\tSAMrecords unvalid\t{c['unvalid']}",
        f"\tSAMrecords mapqv=0\t{c['mapqv0']}",
        f"\tSAMrecords no gene\t{c['no_gene']}",
        f"\tSAMrecords no UMI\t{c['no_umi']}",
        f"\tSAMrecords chimeria\t{c['chimeria']}",
        f"\tTotal reads\t\t{c['reads']}",
        f"\tTotal reads multiSAM\t{c['reads_multi']}",
        "\tMoleculeDataset init start...",
        f"\tTotal molecules\t\t{c['molecules']}",
        f"\tTotal molecule reads\t{c['molecule_reads']}",
        f"\tTotal molecule multiIG\t{c['multi_ig']}",
        "\tSetFusions\t\tstart...",
    ]
    for key, n in sorted(fusions, key=lambda kv: (-kv[1], kv[0].encode("latin-1"))):
        if n >= 10:
            lines.append(f"\t{n} distincts molecules support fusion [{key}]")
    return lines


def output_names(prefix):
    """FusionDetector.java:L107-109"""
    return {sfx: prefix + sfx for sfx in _lib.FUSION_OUTPUTS}


def fusion_detector(ctx, in_bam, csv, outdir, prefix="fusion", segment_bytes=256 << 20, n_threads=4, log=None, host_loop=False, **cfg):
    """-> dict of counts, device ms per stage, bytes written and seconds.  cfg: fields of smi_fusion_config (table_log2, budget_bytes).
    log: a text stream for the reference's messages.  host_loop: also run the reference's single-thread loops on the host
    (host_loop_s, host_loop_mismatches: the baseline of tools/microbench.py)."""
    t_all = time.perf_counter()
    with open(csv, "rb") as f:
        cs = f.read()
    h = _lib.Fusion(ctx, cs, n_threads=n_threads, **cfg)
    t0 = time.perf_counter()
    try:
        for bam, recs, _hdr in segments(in_bam, segment_bytes, n_threads):
            if recs.size:
                h.add_segment(bam, recs)
        t_parse = time.perf_counter() - t0
        t0 = time.perf_counter()
        outs = h.run()
        t_run = time.perf_counter() - t0
        counts = h.counts()
        stage_ms = dict(h.stage_ms)
        base = h.host_loop() if host_loop else None
    finally:
        h.close()
    t0 = time.perf_counter()
    written = 0
    names = output_names(prefix)
    for sfx, data in outs.items():
        with open(os.path.join(outdir, names[sfx]), "wb") as f:
            f.write(data)
        written += len(data)
    fusions = fusions_of(outs["_fusmetrics.txt"])
    if log is not None:
        for line in statistics_lines(counts, fusions):
            print(line, file=log)
    if base is not None:
        counts = dict(counts, host_loop_s=base[0], host_loop_mismatches=base[1])
    return dict(counts, fusions=fusions, stage_ms=stage_ms, bytes_written=written,
                seconds=dict(parse=t_parse, run=t_run, write=time.perf_counter() - t0), wall_s=time.perf_counter() - t_all)
