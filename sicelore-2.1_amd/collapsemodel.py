"""`CollapseModel` (org/ipmc/sicelore/programs/CollapseModel.java:L151-193; the reference README's step 7, "Novel isoform discovery"): the
unassigned (IT = undef) molecules of the ISOBAM that `IsoformMatrix ISOBAM=true` writes, collapsed into novel isoforms per gene.

    java -jar Sicelore-2.1.jar CollapseModel I=isobam.bam CSV=barcodes.csv REFFLAT=genes.refFlat OUTDIR=out PREFIX=CollapseModel

The BAM is read once in segments of about segment_bytes compressed bytes, inflated one segment ahead by a reader thread
(bamsegments.segments) and loaded by the library's host threads (smi_collapse_add_segment), so no .bai is needed and the input need not be
sorted; K-COLLAPSE, K-COLSTAT and K-FILTER / K-CLASS run on the device and the five texts are rendered from their results
(smi_collapse_run).  Genes are in byte order of their name.  A record the loader fails on stops the run before any
file is written.

The validator (UCSCRefFlatParser.validator L279-366) runs when collapse_model is given cage, polya and short and all three exist: the two BED
texts give every transcript its distances on the host, and SHORT, the short-read BAM, is streamed once in segments through K-JSUP, which
counts for every novel junction the records whose alignment blocks have it exactly; it needs no .bai and no sorted input either.  The command
line does not reach it yet: cli.py still refuses a run whose CAGE, POLYA and SHORT all exist, and the follow-up is to lift that refusal and
pass the three paths and the three cut-offs (cageCo, polyaCo, juncCo) through to collapse_model."""
import os
import time

from . import lib as _lib
from .bamsegments import segments


def statistics_lines(c, v=None, cage=None, polya=None):
    """the messages of the reference's run in order (CollapseModel.java:L154, L167 / L173; BEDParser.java:L59; UCSCRefFlatParser.java:L142,
    L207, L213, L286, L293 and statistics L580-591), without the logger's prefix.  v: the validator's counts (Collapse.validate_counts) with
    the CAGE and POLYA paths as given; without them no novel is valid, so the valid set is the gencode one"""
    row = lambda k: f"{c[k]} ({c[k + '_ev']})"  # noqa: E731
    if v is None:
        vrow = lambda k: row(k) if k == "gencode" else "0 (0)"  # noqa: E731
        total = row("gencode")
        validation = ["\tWon't perform validation (please provide CAGE bed, POLYA bed and SHORT read bam files"]
    else:
        vrow = lambda k: f"{v[k + '_valid']} ({v[k + '_valid_ev']})"  # noqa: E731
        total = f"{v['valid_isoforms']} ({v['valid_evidences']})"
        validation = ["\tPerform validation using provided CAGE bed, POLYA bed and SHORT read bam files",
                      f"BEDParser\t{cage}\t[references={v['cage_references']},entries={v['cage_entries']}]",
                      f"BEDParser\t{polya}\t[references={v['polya_references']},entries={v['polya_entries']}]",
                      f"Validator Start...[{c['genes']} total genes]"]
        validation += [f"{nb} genes processed" for nb in range(2500, c["genes"] + 1, 2500)]
    return [
        f"\tCells detected\t\t[{c['cells']}]",
        "Loader Bam Start...",
        f"Loader Bam End...{c['genes']}",
        f"Collapser Start...[{c['genes']} total genes]",
        *validation,
        "Printing statistics...",
        "-----------------------------------------------------------------------",
        "\t\t\t\t\tall_set (UMI)\tvalid_set (UMI)",
        f"total_genes\t\t\t\t{c['genes']}",
        f"total_isoforms\t\t\t\t{c['isoforms']} ({c['evidences']})\t{total}",
        "full_splice_match",
        f" o gencode\t\t\t\t{row('gencode')}\t{vrow('gencode')}",
        "novel_in_catalog",
        f" o combination_of_known_junctions\t{row('ckj')}\t{vrow('ckj')}",
        f" o combination_of_known_splicesites\t{row('cks')}\t{vrow('cks')}",
        "novel_not_in_catalog",
        f" o at_least_one_novel_splicesite\t{row('nss')}\t{vrow('nss')}",
        "------------------------------------------------------------------------",
    ]


def output_names(prefix, delta, rn_min, min_evidence):
    """CollapseModel.java:L177-181"""
    return {sfx: f"{prefix}.d{delta}.rn{rn_min}.e{min_evidence}{sfx}" for sfx in _lib.COLLAPSE_OUTPUTS}


def _short_segments(short, segment_bytes, n_threads):
    """segments over SHORT; a file that is no BGZF stream or no BAM fails by name"""
    it = segments(short, segment_bytes, n_threads)
    while True:
        try:
            seg = next(it)
        except StopIteration:
            return
        except _lib.SmiError as e:
            raise _lib.SmiError(f"SHORT {short}: {e}") from None
        yield seg


def collapse_model(ctx, in_bam, refflat, csv, outdir, prefix="CollapseModel", segment_bytes=256 << 20, n_threads=4, log=None, host_loop=False,
                   cage=None, polya=None, short=None, cage_co=50, polya_co=50, junc_co=1, table_log2=0, **cfg):
    """-> dict of counts, device ms per stage, bytes written and seconds.  cfg: fields of smi_collapse_config (cell_tag, umi_tag, gene_tag,
    iso_tag, rn_tag, max_clip, delta, min_evidence, rn_min, lds_junc).  log: a text stream for the reference's messages.  host_loop: also
    run the reference's single-thread collapse() on the host (host_loop_s, host_loop_mismatches: the baseline of tools/microbench.py).
    cage, polya, short: when all three name existing files (CollapseModel.java:L166) the validator runs with the cut-offs cage_co, polya_co
    and junc_co: SHORT is streamed once in segments through K-JSUP (table_log2: the size of its table, for tests), the files are the
    validated ones and the dict also holds the validator's counts, stage_ms["jsup"] and seconds["short"]."""
    t_all = time.perf_counter()
    with open(refflat, "rb") as f:
        rf = f.read()
    with open(csv, "rb") as f:
        cs = f.read()
    validate = all(p is not None and os.path.exists(p) for p in (cage, polya, short))
    h = None
    t0 = time.perf_counter()
    try:
        for bam, recs, hdr in segments(in_bam, segment_bytes, n_threads):
            if hdr is not None:                       # the @SQ dictionary comes with the first segment
                _text, refs, _start = _lib.bam_header(bam)
                h = _lib.Collapse(ctx, rf, cs, [r[0] for r in refs], n_threads=n_threads, **cfg)
            if recs.size:
                h.add_segment(bam, recs)
        t_parse = time.perf_counter() - t0
        t0 = time.perf_counter()
        outs = h.run()
        t_run = time.perf_counter() - t0
        seconds = dict(parse=t_parse, run=t_run)
        vcounts = None
        if validate:
            t0 = time.perf_counter()
            with open(cage, "rb") as f:
                cg = f.read()
            with open(polya, "rb") as f:
                pa = f.read()
            for bam, recs, hdr in _short_segments(short, segment_bytes, n_threads):
                if hdr is not None:
                    _text, refs, _start = _lib.bam_header(bam)
                    h.validate_begin(cg, pa, [r[0] for r in refs], cage_co, polya_co, junc_co, table_log2)
                if recs.size:
                    h.validate_segment(bam, recs)
            outs = h.validate_end()
            vcounts = h.validate_counts()
            seconds["short"] = time.perf_counter() - t0
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
        for line in statistics_lines(counts, vcounts, cage, polya):
            print(line, file=log)
    if vcounts is not None:
        counts = dict(counts, **vcounts)
    if base is not None:
        counts = dict(counts, host_loop_s=base[0], host_loop_mismatches=base[1])
    return dict(counts, stage_ms=stage_ms, bytes_written=written, seconds=dict(seconds, write=time.perf_counter() - t0),
                wall_s=time.perf_counter() - t_all)
