"""`ExportClippedReads` (org/ipmc/sicelore/programs/ExportClippedReads.java:L50-104) and `AddBamReadTags` (AddBamReadTags.java:L38-72): the
two programs in front of `FusionDetector` in the reference README's step 6, "Fusion transcripts detection cell by cell".

    python sicelore-2.1_amd/fusionprep.py ExportClippedReads I=passedParsedWithSequences.bam O=clipped_reads.fastq [MINCLIP=150] ...
    (minimap2, samtools: the clipped reads mapped again -- outside tools, like every mapping step)
    python sicelore-2.1_amd/fusionprep.py AddBamReadTags I=clipped_reads.bam O=clipped_reads.tags.bam [GENETAG=GE] [CELLTAG=BC] [UMITAG=U8]

Both take Picard's two syntaxes (`-I x` and `I=x`).  They have a command line of their own: `cli.main`, `python sicelore-2.1_amd` and
`bin/java` keep refusing the two names (DESIGN.md sections 8k and 9).

The BAM is read in segments (bamsegments.segments).  ExportClippedReads: K-CLIP-FLAG / K-CLIP-KEY / K-CLIP-INSERT / K-CLIP-WRITE give a
segment's FASTQ text (smi_clipexport_segment), the table of the keys written staying on the device between segments.  AddBamReadTags:
K-NAME's `_` form decides the three edits of a record and K-EDIT writes it (smi_moltag_segment, SMI_MOLTAG_READ), through the writer of
AddBamMoleculeTags (moltags._rewrite).  The output goes to a temporary file beside OUTPUT that takes OUTPUT's name once the last segment is
written: a record on which the reference's loop dies raises lib.ClipExportError and leaves no file."""
import os
import sys
import time

if __name__ == "__main__" and "sicelore_amd" not in sys.modules:      # run as a file: the package under the name the repository uses for it
    import importlib.util
    _HERE = os.path.dirname(os.path.abspath(__file__))
    _spec = importlib.util.spec_from_file_location("sicelore_amd", os.path.join(_HERE, "__init__.py"), submodule_search_locations=[_HERE])
    _mod = importlib.util.module_from_spec(_spec)
    sys.modules["sicelore_amd"] = _mod
    _spec.loader.exec_module(_mod)
    from sicelore_amd import fusionprep as _self
    sys.exit(_self.main())

from . import lib as _lib
from .bamsegments import segments


def export_clipped_reads(ctx, in_bam, out_fastq, min_clip=150, cell_tag="BC", umi_tag="U8", gene_tag="GE", us_tag="US", qs_tag="QS",
                         segment_bytes=256 << 20, n_threads=4, table_log2=0, host_loop=False):
    """-> dict of counts (records, clipped, written, ...), device ms per stage, seconds and bytes written.  table_log2: the starting size
    of the key table, for tests.  host_loop: also run the reference's single-thread loop on the host (host_loop_s, host_loop_mismatches:
    the baseline of tools/microbench.py)."""
    t_all = time.perf_counter()
    h = _lib.ClipExport(ctx, min_clip=min_clip, cell_tag=cell_tag, umi_tag=umi_tag, gene_tag=gene_tag, us_tag=us_tag, qs_tag=qs_tag,
                        table_log2=table_log2, keep_records=host_loop)
    tmp = f"{out_fastq}.tmp{os.getpid()}"
    written = 0
    secs = dict(device=0.0, write=0.0)
    stage_ms = dict.fromkeys(_lib.CLIPEXPORT_STAGES, 0.0)
    try:
        with open(tmp, "wb") as f:
            for bam, recs, _hdr in segments(in_bam, segment_bytes, n_threads):
                if not recs.size:
                    continue
                t0 = time.perf_counter()
                out = h.segment(bam, recs)
                t1 = time.perf_counter()
                f.write(memoryview(out))
                secs["device"] += t1 - t0
                secs["write"] += time.perf_counter() - t1
                written += out.size
                for k, v in h.stage_ms().items():
                    stage_ms[k] += v
        counts = h.counts()
        if host_loop:
            counts["host_loop_s"], counts["host_loop_mismatches"] = h.host_loop()
        os.replace(tmp, out_fastq)
    finally:
        h.close()
        if os.path.exists(tmp):
            os.remove(tmp)
    wall = time.perf_counter() - t_all
    secs["parse"] = max(0.0, wall - secs["device"] - secs["write"])       # reading, inflating and indexing the segments
    return dict(counts, stage_ms=stage_ms, seconds=secs, bytes_written=written, wall_s=wall)


def add_bam_read_tags(ctx, in_bam, out_bam, gene_tag="GE", cell_tag="BC", umi_tag="U8", segment_bytes=256 << 20, n_threads=4, index=False):
    """-> dict of counts (records, tagged), device ms per stage, seconds and bytes written.  The header is copied as it is (presorted =
    true, L44).  index: also leave <out_bam>.bai (moltags._rewrite)."""
    from .moltags import _rewrite
    h = _lib.MolTag(ctx, _lib.MOLTAG_READ, gene_tag=gene_tag, cell_tag=cell_tag, umi_tag=umi_tag)
    try:
        info = _rewrite(ctx, h, in_bam, out_bam, lambda hdr: hdr, segment_bytes, n_threads, index=index)
    finally:
        h.close()
    info["seconds"]["parse"] = max(0.0, info["wall_s"] - sum(info["seconds"].values()))      # reading, inflating and indexing the segments
    return info


# Picard's option names -> (keyword of the function or None, kind, default) (ExportClippedReads.java:L25-40, AddBamReadTags.java:L22-31)
EC_OPTIONS = {
    "I": (None, "path", None), "O": (None, "path", None), "MINCLIP": ("min_clip", "int", 150), "CELLTAG": ("cell_tag", "tag", "BC"),
    "UMITAG": ("umi_tag", "tag", "U8"), "GENETAG": ("gene_tag", "tag", "GE"), "USTAG": ("us_tag", "tag", "US"), "QSTAG": ("qs_tag", "tag", "QS"),
    "VALIDATION_STRINGENCY": (None, "stringency", "STRICT"),
}
RT_OPTIONS = {
    "I": (None, "path", None), "O": (None, "path", None), "GENETAG": ("gene_tag", "tag", "GE"), "CELLTAG": ("cell_tag", "tag", "BC"),
    "UMITAG": ("umi_tag", "tag", "U8"), "VALIDATION_STRINGENCY": (None, "stringency", "STRICT"),
}
LONG = {"INPUT": "I", "OUTPUT": "O"}


def exportclippedreads(argv):
    """ExportClippedReads.doWork (L50-104).  O is optional in the reference, which then opens it (L62): a missing O is an argument error.
    VALIDATION_STRINGENCY is accepted and changes nothing."""
    from . import cli
    prog = "ExportClippedReads"
    o = cli._picard_parse(argv, prog, EC_OPTIONS, LONG)
    need = [k for k in ("I", "O") if k not in o]
    if need:
        raise cli.CliError(f"sub-command {prog}: missing required option(s) {', '.join(need)}")
    if not os.path.isfile(o["I"]):                                          # IOUtil.assertFileIsReadable (L55)
        raise cli.CliError(f"{prog}: I={o['I']}: no such file")
    if not os.path.isdir(os.path.dirname(os.path.abspath(o["O"]))) or os.path.isdir(o["O"]):   # IOUtil.assertFileIsWritable (L56)
        raise cli.CliError(f"{prog}: O={o['O']}: no such directory, or a directory")
    cfg = {f: o.get(k, d) for k, (f, _kind, d) in EC_OPTIONS.items() if f is not None}
    if not -2 ** 31 <= cfg["min_clip"] < 2 ** 31:                           # a Java int
        raise cli.CliError(f"sub-command {prog}: MINCLIP {cfg['min_clip']!r} is not a number")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise cli.CliError(f"{prog} runs in one process on one GPU in this build: start it without torchrun")
    try:
        info = export_clipped_reads(cli._context(), o["I"], o["O"], n_threads=cli._ncpu({}), **cfg)
    except _lib.ClipExportError as e:
        raise cli.CliError(f"{prog}: record {e.record}: {e}; {o['O']} was not written (the reference stops reading there, leaves a cut-off "
                           "file and exits 0)")
    print(f"DONE -- {info['records']} records, {info['clipped']} of them clipped, {info['written']} written", file=sys.stderr)
    return 0


def addbamreadtags(argv):
    """AddBamReadTags.doWork (L38-72).  VALIDATION_STRINGENCY is accepted and changes nothing."""
    from . import cli
    o, cfg = cli._moltag_options(argv, "AddBamReadTags", RT_OPTIONS, ("I",))
    info = add_bam_read_tags(cli._context(), o["I"], o["O"], n_threads=cli._ncpu({}), **cfg)
    print(f"DONE -- {info['records']} records, {info['tagged']} of them tagged", file=sys.stderr)
    return 0


def main(argv=None):
    """-> exit code: 0, or 1 with the message on stderr (argument errors, and the records ExportClippedReads stops at, named)"""
    from . import cli
    argv = list(sys.argv[1:] if argv is None else argv)
    try:
        if not argv or argv[0] in ("-h", "--help", "help"):
            print(__doc__)
            return 0
        sub, rest = argv[0], argv[1:]
        if sub == "ExportClippedReads":
            return exportclippedreads(rest)
        if sub == "AddBamReadTags":
            return addbamreadtags(rest)
        raise cli.CliError(f"sub-command {sub!r}: fusionprep.py has ExportClippedReads and AddBamReadTags")
    except cli.CliError as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return 1
    except (_lib.SmiError, OSError, ValueError) as e:
        print(f"ERROR: {type(e).__name__}: {e}", file=sys.stderr)
        return 1
