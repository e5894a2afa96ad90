"""`ComputeConsensus` (org/ipmc/sicelore/programs/ComputeConsensus.java:L67-107; sicelore-nf/main.nf:156): one consensus FASTQ record per
molecule (cell barcode + UMI) of a BAM whose records carry their read's sequence (tagbamwithread's US).

    java -jar Sicelore-2.1.jar ComputeConsensus -T 16 -I chromosome.bam -O chr.fq -CELLTAG BC -UMITAG U8 ... -MAXREADS 20 -MINPS 3 -MAXPS 20

The BAM is read in segments of about segment_bytes compressed bytes (bamsegments.segments) and parsed by the
library's host threads (smi_consensus_add_segment); the kept records of the whole input stay in memory, as in the reference (main.nf
splits the input per chromosome).  Molecules of 3 or more selected reads are aligned by K-POA on the device (smi_consensus_run); the FASTQ
is written plain, molecules in the order of their first kept record."""
import time

from . import lib as _lib
from .bamsegments import segments


def compute_consensus(ctx, in_bam, out_fastq, segment_bytes=256 << 20, n_threads=4, **cfg):
    """-> dict of the parser's counts, seconds per phase and K-POA device ms.  cfg: fields of smi_consensus_config (cell_tag, umi_tag,
    gene_tag, tso_end_tag, polya_start_tag, cdna_tag, us_tag, rn_tag, max_clip, mapqv0, max_reads, min_ps, max_ps, scratch_bytes)."""
    t_all = time.perf_counter()
    secs = dict(bam_read_inflate=0.0, index=0.0, parse=0.0, consensus=0.0, write=0.0)
    h = _lib.Consensus(ctx, n_threads=n_threads, **cfg)
    try:
        for bam, recs, _hdr in segments(in_bam, segment_bytes, n_threads, secs):
            t1 = time.perf_counter()
            if recs.size:
                h.add_segment(bam, recs)
            secs["parse"] += time.perf_counter() - t1
        t1 = time.perf_counter()
        fastq = h.run()
        secs["consensus"] = time.perf_counter() - t1
        t1 = time.perf_counter()
        with open(out_fastq, "wb") as f:
            f.write(fastq)
        secs["write"] = time.perf_counter() - t1
        counts = h.counts()
        kernel_ms = h.kernel_ms
    finally:
        h.close()
    return dict(counts, seconds=secs, poa_kernel_ms=kernel_ms, wall_s=time.perf_counter() - t_all)


def parser_log(counts):
    """the parser's and the dataset's counts as LongreadParser (L85-93) and MoleculeDataset (L85) log them"""
    return "\n".join([
        f"\tTotal SAMrecords\t{counts['records']}", f"\tSAMrecords valid\t{counts['valid']}", f"\tSAMrecords unvalid\t{counts['unvalid']}",
        f"\tSAMrecords mapqv=0\t{counts['mapqv0']}", f"\tSAMrecords no gene\t{counts['no_gene']}", f"\tSAMrecords no UMI\t{counts['no_umi']}",
        f"\tSAMrecords chimeria\t{counts['chimeria']}", f"\tTotal reads\t\t{counts['reads']}", f"\tTotal reads multiSAM\t{counts['reads_multi']}",
        f"\tTotal molecules\t\t{counts['molecules']}"])
