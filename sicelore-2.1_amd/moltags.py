"""`AddBamMoleculeTags` (org/ipmc/sicelore/programs/AddBamMoleculeTags.java:L38-67; sicelore-nf/main.nf:217) and `AddGeneNameTag`
(AddGeneNameTag.java:L76-160; main.nf:235): a molecule BAM rewritten record by record with BC / U8 / RN from the read names, then with
GE / GS / XF from a refFlat gene model.

    java -jar Sicelore-2.1.jar AddBamMoleculeTags -I molecules.bam -O molecules.tags.bam [-CELLTAG BC] [-UMITAG U8] [-RNTAG RN]
    java -jar Sicelore-2.1.jar AddGeneNameTag -I molecules.tags.bam -O molecules.tags.GE.bam -REFFLAT genes.refFlat [-GENETAG GE] ...

The BAM is read in segments (bamsegments.segments); K-NAME / K-GENE decide the edits of a segment and K-EDIT writes its records
(smi_moltag_segment), which are deflated on the device into BGZF blocks and followed by the EOF block, as ISOBAM is written.  The output
goes to a temporary file beside OUTPUT that takes OUTPUT's name once the last segment is written: a record on which the reference's loop
dies raises lib.MolTagError and leaves no file."""
import os
import time

import numpy as np

from . import lib as _lib
from .bamsegments import BGZF_EOF, segments
from .isoformmatrix import isobam_header


def _rewrite(ctx, h, in_bam, out_bam, header, segment_bytes, n_threads, index=False):
    """index: also leave <out_bam>.bai, built from the records and the BGZF blocks as they are written (bamindex.WriterIndex); the info
    then has `index` (its counts and times; None when the output is not in coordinate order: the BAM is kept and `index_error` says why)"""
    t_all = time.perf_counter()
    tmp = f"{out_bam}.tmp{os.getpid()}"
    written = 0
    secs = dict(device=0.0, deflate=0.0, write=0.0)
    stage_ms = dict.fromkeys(_lib.MOLTAG_STAGES, 0.0)
    wix = None
    if index:
        from .bamindex import WriterIndex
        wix = WriterIndex(ctx)
    try:
        with open(tmp, "wb") as f:
            def emit(data, records=True):
                t0 = time.perf_counter()
                z = ctx.bgzf_deflate_device(np.frombuffer(data, dtype=np.uint8) if isinstance(data, bytes) else data)
                t1 = time.perf_counter()
                f.write(memoryview(z[:-28]))
                secs["deflate"] += t1 - t0
                secs["write"] += time.perf_counter() - t1
                if wix is not None:
                    wix.emitted(data, z[:-28], written, records)
                return len(z) - 28
            for bam, recs, hdr in segments(in_bam, segment_bytes, n_threads):
                if hdr is not None:
                    written += emit(header(hdr), records=False)
                if recs.size:
                    t0 = time.perf_counter()
                    out = h.segment(bam, recs)
                    secs["device"] += time.perf_counter() - t0
                    for k, v in h.stage_ms().items():
                        stage_ms[k] += v
                    written += emit(out)
            f.write(BGZF_EOF)
            written += len(BGZF_EOF)
        os.replace(tmp, out_bam)
        info = dict(h.counts(), stage_ms=stage_ms, seconds=secs, bytes_written=written)
        if wix is not None:
            info["index"], info["index_error"] = wix.finish(f"{out_bam}.bai", written - len(BGZF_EOF))
    finally:
        if wix is not None:
            wix.close()
        if os.path.exists(tmp):
            os.remove(tmp)
    info["wall_s"] = time.perf_counter() - t_all
    return info


def add_bam_molecule_tags(ctx, in_bam, out_bam, cell_tag="BC", umi_tag="U8", rn_tag="RN", segment_bytes=256 << 20, n_threads=4, index=False):
    """-> dict of counts, device ms per stage, seconds and bytes written.  The header is copied as it is (presorted = true, L44).
    index: also leave <out_bam>.bai, in the place of the `samtools index` the scripts run next (_rewrite)."""
    h = _lib.MolTag(ctx, _lib.MOLTAG_MOLECULE, cell_tag=cell_tag, umi_tag=umi_tag, rn_tag=rn_tag)
    try:
        return _rewrite(ctx, h, in_bam, out_bam, lambda hdr: hdr, segment_bytes, n_threads, index=index)
    finally:
        h.close()


METRICS = "TOTAL READS [{total_reads}] CORRECT_STRAND [{right_strand}]  WRONG_STRAND [{wrong_strand}] AMBIGUOUS_STRAND_FIXED [{ambiguous_fixed}] " \
          "AMBIGUOUS REJECTED READS [{ambiguous_rejected}]"          # ReadTaggingMetric.toString, AddGeneNameTag.java:L407


def add_gene_name_tag(ctx, in_bam, out_bam, refflat, gene_tag="GE", strand_tag="GS", function_tag="XF", use_strand_info=True,
                      allow_multi_gene_reads=True, segment_bytes=256 << 20, n_threads=4, log=None, index=False):
    """-> dict of counts (the five metrics among them), device ms per stage, seconds and bytes written.  The header gets SO:unsorted (L80)
    as ISOBAM's does.  log: a text stream for `Loaded <n> transcripts.` (L84) and the metrics line (L113).  index: also leave
    <out_bam>.bai (_rewrite); the records keep the input's order, and the index follows the records, not the header's SO."""
    with open(refflat, "rb") as f:
        rf = f.read()
    with open(in_bam, "rb") as f:                      # the reference dictionary comes first: the model keeps the genes on its sequences
        head = np.frombuffer(f.read(int(min(segment_bytes, 64 << 20))), dtype=np.uint8)
    hdr_bytes, _used = _lib.bgzf_inflate(head, n_threads=n_threads)
    _text, refs, _start = _lib.bam_header(hdr_bytes)
    genes = _lib.GeneTagger(rf, [r[0] for r in refs])
    h = None
    try:
        h = _lib.MolTag(ctx, _lib.MOLTAG_GENE, genes=genes, gene_tag=gene_tag, strand_tag=strand_tag, function_tag=function_tag,
                        use_strand_info=use_strand_info, allow_multi_gene_reads=allow_multi_gene_reads)
        if log is not None:
            print(f"Loaded {genes.n_genes} transcripts.", file=log)
        info = _rewrite(ctx, h, in_bam, out_bam, isobam_header, segment_bytes, n_threads, index=index)
        if log is not None:
            print(METRICS.format(**info), file=log)
        return info
    finally:
        if h is not None:
            h.close()
        genes.close()
