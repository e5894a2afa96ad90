"""`CollapseModel` (org/ipmc/sicelore/programs/CollapseModel.java:L151-193; the reference README's step 7, "Novel isoform discovery"): the
unassigned (IT = undef) molecules of the ISOBAM that `IsoformMatrix ISOBAM=true` writes, collapsed into novel isoforms per gene.

    java -jar Sicelore-2.1.jar CollapseModel I=isobam.bam CSV=barcodes.csv REFFLAT=genes.refFlat OUTDIR=out PREFIX=CollapseModel

The BAM is read once in segments of about segment_bytes compressed bytes, inflated one segment ahead by a reader thread
(isoformmatrix._segments) and loaded by the library's host threads (smi_collapse_add_segment), so no .bai is needed and the input need not be
sorted; K-COLLAPSE, K-COLSTAT and K-FILTER / K-CLASS run on the device and the five texts are rendered from their results
(smi_collapse_run).  Genes are in byte order of their name.  A record the loader fails on stops the run before any
file is written.  The validator (CAGE, POLYA, SHORT) is not part of this build: cli.py refuses a run that would need it."""
import os
import time

from . import lib as _lib
from .isoformmatrix import _segments


def statistics_lines(c):
    """the messages of the reference's run in order (CollapseModel.java:L154, L173; UCSCRefFlatParser.java:L142, L207, L213 and statistics
    L580-591), without the logger's prefix; no novel is valid without the validator, so the valid set is the gencode one"""
    row = lambda k: f"{c[k]} ({c[k + '_ev']})"  # noqa: E731
    return [
        f"\tCells detected\t\t[{c['cells']}]",
        "Loader Bam Start...",
        f"Loader Bam End...{c['genes']}",
        f"Collapser Start...[{c['genes']} total genes]",
        "\tWon't perform validation (please provide CAGE bed, POLYA bed and SHORT read bam files",
        "Printing statistics...",
        "-----------------------------------------------------------------------",
        "\t\t\t\t\tall_set (UMI)\tvalid_set (UMI)",
        f"total_genes\t\t\t\t{c['genes']}",
        f"total_isoforms\t\t\t\t{c['isoforms']} ({c['evidences']})\t{row('gencode')}",
        "full_splice_match",
        f" o gencode\t\t\t\t{row('gencode')}\t{row('gencode')}",
        "novel_in_catalog",
        f" o combination_of_known_junctions\t{row('ckj')}\t0 (0)",
        f" o combination_of_known_splicesites\t{row('cks')}\t0 (0)",
        "novel_not_in_catalog",
        f" o at_least_one_novel_splicesite\t{row('nss')}\t0 (0)",
        "------------------------------------------------------------------------",
    ]


def output_names(prefix, delta, rn_min, min_evidence):
    """CollapseModel.java:L177-181"""
    return {sfx: f"{prefix}.d{delta}.rn{rn_min}.e{min_evidence}{sfx}" for sfx in _lib.COLLAPSE_OUTPUTS}


def collapse_model(ctx, in_bam, refflat, csv, outdir, prefix="CollapseModel", segment_bytes=256 << 20, n_threads=4, log=None, host_loop=False,
                   **cfg):
    """-> dict of counts, device ms per stage, bytes written and seconds.  cfg: fields of smi_collapse_config (cell_tag, umi_tag, gene_tag,
    iso_tag, rn_tag, max_clip, delta, min_evidence, rn_min, lds_junc).  log: a text stream for the reference's messages.  host_loop: also
    run the reference's single-thread collapse() on the host (host_loop_s, host_loop_mismatches: the baseline of tools/microbench.py)."""
    t_all = time.perf_counter()
    with open(refflat, "rb") as f:
        rf = f.read()
    with open(csv, "rb") as f:
        cs = f.read()
    h = None
    t0 = time.perf_counter()
    try:
        for bam, recs, hdr in _segments(in_bam, segment_bytes, n_threads):
            if hdr is not None:                       # the @SQ dictionary comes with the first segment
                _text, refs, _start = _lib.bam_header(bam)
                h = _lib.Collapse(ctx, rf, cs, [r[0] for r in refs], n_threads=n_threads, **cfg)
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
        if h is not None:
            h.close()
    t0 = time.perf_counter()
    written = 0
    names = output_names(prefix, cfg.get("delta", 2), cfg.get("rn_min", 1), cfg.get("min_evidence", 2))
    for sfx, data in outs.items():
        with open(os.path.join(outdir, names[sfx]), "wb") as f:
            f.write(data)
        written += len(data)
    if log is not None:
        for line in statistics_lines(counts):
            print(line, file=log)
    if base is not None:
        counts = dict(counts, host_loop_s=base[0], host_loop_mismatches=base[1])
    return dict(counts, stage_ms=stage_ms, bytes_written=written, seconds=dict(parse=t_parse, run=t_run, write=time.perf_counter() - t0),
                wall_s=time.perf_counter() - t_all)
