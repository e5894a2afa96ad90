"""`IsoformMatrix` (org/ipmc/sicelore/programs/IsoformMatrix.java:L93-160; quickrun-2.1.sh:46, sicelore-nf/main.nf:99 and :252): the cell x
isoform, cell x gene and cell x junction matrices of a molecule-tagged BAM, STRICT method.

    java -jar Sicelore-2.1.jar IsoformMatrix -I in.bam -REFFLAT genes.refFlat -CSV barcodes.csv -OUTDIR out -PREFIX sicelore [-DELTA 2] ...

The BAM is read in segments of about segment_bytes compressed bytes (bamsegments.segments) and parsed by the
library's host threads (smi_isoform_add_segment); K-ISO assigns the molecules and K-MTX counts and renders the matrices on the device
(smi_isoform_run).  Rows and columns are in byte order and molinfos in (cell, UMI) order.  With ISOBAM a second
pass over the BAM writes PREFIX_isobam.bam: every record with IG / IT, assembled on the device (smi_isoform_isobam), behind the input's
header with SO:unsorted.  PREFIX.html and histogram.png (JFreeChart) are not written."""
import os
import struct
import time

import numpy as np

from . import lib as _lib
from .bamsegments import BGZF_EOF, segments


def unsorted_header(text):
    """samFileHeader.setSortOrder(unsorted) as this build writes it: SO:unsorted in the @HD line -- an SO value
    replaced in place, else appended to the line; a header without @HD gets `@HD\tVN:1.6\tSO:unsorted` in front.  Other lines verbatim."""
    lines = text.split("\n")
    if lines and lines[0].startswith("@HD"):
        f = lines[0].split("\t")
        for i in range(1, len(f)):
            if f[i].startswith("SO:"):
                f[i] = "SO:unsorted"
                break
        else:
            f.append("SO:unsorted")
        lines[0] = "\t".join(f)
        return "\n".join(lines)
    return "@HD\tVN:1.6\tSO:unsorted\n" + text


def isobam_header(hdr):
    """the input's header bytes (magic, text, references) with the text of unsorted_header"""
    l_text = struct.unpack_from("<I", hdr, 4)[0]
    text = unsorted_header(hdr[8:8 + l_text].decode("latin-1")).encode("latin-1")
    return b"BAM\1" + struct.pack("<I", len(text)) + text + hdr[8 + l_text:]


def isoform_matrix(ctx, in_bam, refflat, csv, outdir, prefix="sicelore", segment_bytes=256 << 20, n_threads=4, log_params=None, isobam=False,
                   **cfg):
    """-> dict of counts, device ms per stage, bytes written and seconds.  cfg: fields of smi_isoform_config (cell_tag, umi_tag, gene_tag,
    rn_tag, max_clip, mapqv0, delta, to_bulk, lds_tx, budget_bytes).  log_params: the option lines of PREFIX.log (writeLOGS), in order.
    isobam: also PREFIX_isobam.bam (BGZF, blocks deflated on the device)."""
    t_all = time.perf_counter()
    with open(refflat, "rb") as f:
        rf = f.read()
    with open(csv, "rb") as f:
        cs = f.read()
    h = _lib.Isoform(ctx, rf, cs, n_threads=n_threads, **cfg)
    try:
        t0 = time.perf_counter()
        for bam, recs, _hdr in segments(in_bam, segment_bytes, n_threads):
            if recs.size:
                h.add_segment(bam, recs)
        t_parse = time.perf_counter() - t0
        t0 = time.perf_counter()
        outs = h.run()
        t_run = time.perf_counter() - t0
        counts = h.counts()
        stage_ms = dict(h.stage_ms)
        t0 = time.perf_counter()
        isobam_bytes = 0
        if isobam:                                   # IsoformMatrix.java:L135-159: a second pass over every record
            with open(os.path.join(outdir, f"{prefix}_isobam.bam"), "wb") as f:
                def emit(data):
                    z = ctx.bgzf_deflate_device(np.frombuffer(data, dtype=np.uint8) if isinstance(data, bytes) else data)
                    f.write(memoryview(z[:-28]))
                    return len(z) - 28
                for bam, recs, hdr in segments(in_bam, segment_bytes, n_threads):
                    if hdr is not None:
                        isobam_bytes += emit(isobam_header(hdr))
                    if recs.size:
                        isobam_bytes += emit(h.isobam(bam, recs))
                f.write(BGZF_EOF)
                isobam_bytes += len(BGZF_EOF)
        t_isobam = time.perf_counter() - t0
    finally:
        h.close()
    t0 = time.perf_counter()
    written = 0
    for name, data in outs.items():
        if name.startswith("bulk") and not cfg.get("to_bulk"):
            continue
        with open(os.path.join(outdir, f"{prefix}_{name}"), "wb") as f:
            f.write(data)
        written += len(data)
    log = write_log_text(log_params or [], counts).encode()
    with open(os.path.join(outdir, f"{prefix}.log"), "wb") as f:
        f.write(log)
    written += len(log) + isobam_bytes
    return dict(counts, stage_ms=stage_ms, bytes_written=written, seconds=dict(parse=t_parse, run=t_run, isobam=t_isobam,
                                                                              write=time.perf_counter() - t0),
                wall_s=time.perf_counter() - t_all)


def write_log_text(params, c):
    """IsoformMatrix.writeLOGS (L162-210): params = [(name, value text)] for the IsoformMatrix lines, then the counters"""
    lines = [f"IsoformMatrix {k},{v}" for k, v in params]
    lines += [
        f"Total SAMrecords,{c['records']}", f"SAMrecords valid,{c['valid']}", f"SAMrecords unvalid,{c['unvalid']}",
        f"SAMrecords mapqv=0,{c['mapqv0']}", f"SAMrecords no gene,{c['no_gene']}", f"SAMrecords no UMI,{c['no_umi']}",
        f"SAMrecords chimeria,{c['chimeria']}", f"Total reads,{c['reads']}", f"Total reads multiSAM,{c['reads_multi']}",
        f"Total molecules,{c['molecules']}", f"Total molecule reads,{c['molecule_reads']}", f"Total molecule multiIG,{c['multi_ig']}",
        f"UCSCRefFlatParser genes,{c['genes']}", f"UCSCRefFlatParser transcripts,{c['transcripts']}",
        f"SetIsoforms monoexon,{c['monoexon']}", f"SetIsoforms no match,{c['nomatch']}", f"SetIsoforms one match,{c['onematch']}",
        f"SetIsoforms ambiguous,{c['ambiguous']}", f"Matrix cells size,{c['cells']}", f"Matrix genes size,{c['matrix_genes']}",
        f"Matrix junctions size,{c['matrix_junctions']}", f"Matrix isoforms size,{c['matrix_isoforms']}",
        f"Matrix isoforms counts,{c['total_count']}", f"Matrix isoforms define,{c['isoforms_def']}",
        f"Matrix isoforms undefined,{c['isoforms_undef']}"]
    return "".join(x + "\n" for x in lines)
