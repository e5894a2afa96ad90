"""`SNPMatrix` (org/ipmc/sicelore/programs/SNPMatrix.java:L72-216; the reference README's step 5, "Single Nucleotide Variant calling cell
by cell"): the cell x SNP / editing-site matrix of a molecule BAM.

    java -jar Sicelore-2.1.jar SNPMatrix I=molecules.GE.tags.bam MINRN=0 MINQV=0 CSV=barcodes.csv SNP=snps.csv O=. PREFIX=snp

The BAM is read once in segments of about segment_bytes compressed bytes, inflated one segment ahead by a reader thread
(bamsegments.segments); K-SNP evaluates every site line against every record of a segment on the device (smi_snp_add_segment), so no
.bai is needed and the input need not be sorted; the distinct UMIs per (row, cell) are counted and the dense matrix is rendered on the
device (smi_snp_run).  Rows and cells are in byte order, molinfos in SNP-file line order, then BAM record order.
PREFIX_snpmatrix.txt, PREFIX_snpmetrics.txt and PREFIX_snpmolinfos.txt are written only when at least one row exists."""
import os
import re
import time

from . import lib as _lib
from .bamsegments import segments

NOTHING = ("end of processing...\tnothing has been detected, check your input parameters (if Illumina set CELLBC=CB UMITAG=UB), "
           "no output files generated\t")


def snp_lines(text):
    """the lines SNPMatrix reads (BufferedReader.readLine until the end or the first empty line, L101-102)"""
    lines = re.split("\r\n|\r|\n", text)
    if lines and lines[-1] == "":
        lines.pop()
    out = []
    for line in lines:
        if line == "":
            break
        out.append(line)
    return out


def snp_matrix(ctx, in_bam, csv, snp, outdir, prefix="snp", min_rn=0, min_qv=0, segment_bytes=256 << 20, n_threads=4, log=None, **cfg):
    """-> dict of counts, per-line counts, device ms per stage, bytes written and seconds.  cfg: fields of smi_snp_config (cell_tag, umi_tag,
    gene_tag, rn_tag, max_clip, budget_bytes).  log: a text stream for the reference's `processing...` / `STATISTICS...` lines."""
    t_all = time.perf_counter()
    with open(snp, "rb") as f:
        snp_text = f.read()
    with open(csv, "rb") as f:
        cs = f.read()
    h = None
    t0 = time.perf_counter()
    try:
        for bam, recs, hdr in segments(in_bam, segment_bytes, n_threads):
            if hdr is not None:                       # the @SQ dictionary comes with the first segment
                _text, refs, _start = _lib.bam_header(bam)
                h = _lib.Snp(ctx, snp_text, cs, [r[0] for r in refs], min_rn=min_rn, min_qv=min_qv, n_threads=n_threads, **cfg)
            if recs.size:
                h.add_segment(bam, recs)
        t_scan = time.perf_counter() - t0
        t0 = time.perf_counter()
        outs = h.run()
        t_run = time.perf_counter() - t0
        counts = h.counts()
        per_line = h.line_counts()
        stage_ms = dict(h.stage_ms)
    finally:
        if h is not None:
            h.close()
    lines = snp_lines(snp_text.decode("latin-1"))
    line_counts = [dict(line=ln, hits=int(c[0]), lowRN=int(c[1]), lowQV=int(c[2])) for ln, c in zip(lines, per_line) if c[0] >= 0]
    t0 = time.perf_counter()
    written = 0
    if counts["rows"] > 0:
        for name, data in outs.items():
            with open(os.path.join(outdir, f"{prefix}_{name}"), "wb") as f:
                f.write(data)
            written += len(data)
    if log is not None:
        print(f"Cells detected\t\t[{counts['cells']}]", file=log)
        for c in line_counts:
            print(f"processing...\t\t{c['line']}\t{c['hits']} hits, {c['lowRN']} lowRN, {c['lowQV']} lowQV", file=log)
        if counts["rows"] == 0:
            print(NOTHING, file=log)
        print(f"STATISTICS...\t\thits={counts['hits']}, lowRN={counts['lowRN']}, lowQV= {counts['lowQV']}", file=log)
    return dict(counts, line_counts=line_counts, stage_ms=stage_ms, bytes_written=written,
                seconds=dict(scan=t_scan, run=t_run, write=time.perf_counter() - t0), wall_s=time.perf_counter() - t_all)
