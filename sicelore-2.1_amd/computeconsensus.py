"""`ComputeConsensus` (org/ipmc/sicelore/programs/ComputeConsensus.java:L67-107; sicelore-nf/main.nf:156): one consensus FASTQ record per
molecule (cell barcode + UMI) of a BAM whose records carry their read's sequence (tagbamwithread's US).

    java -jar Sicelore-2.1.jar ComputeConsensus -T 16 -I chromosome.bam -O chr.fq -CELLTAG BC -UMITAG U8 ... -MAXREADS 20 -MINPS 3 -MAXPS 20

The BAM is read in segments of about segment_bytes compressed bytes, inflated one segment ahead by a reader thread and parsed by the
library's host threads (smi_consensus_add_segment); the kept records of the whole input stay in memory, as in the reference (main.nf
splits the input per chromosome).  Molecules of 3 or more selected reads are aligned by K-POA on the device (smi_consensus_run); the FASTQ
is written plain, molecules in the order of their first kept record."""
import queue
import threading
import time

import numpy as np

from . import lib as _lib


def compute_consensus(ctx, in_bam, out_fastq, segment_bytes=256 << 20, n_threads=4, **cfg):
    """-> dict of the parser's counts, seconds per phase and K-POA device ms.  cfg: fields of smi_consensus_config (cell_tag, umi_tag,
    gene_tag, tso_end_tag, polya_start_tag, cdna_tag, us_tag, rn_tag, max_clip, mapqv0, max_reads, min_ps, max_ps, scratch_bytes)."""
    t_all = time.perf_counter()
    secs = dict(bam_read_inflate=0.0, index=0.0, parse=0.0, consensus=0.0, write=0.0)
    h = _lib.Consensus(ctx, n_threads=n_threads, **cfg)
    segments = queue.Queue(maxsize=1)

    def reader():
        try:
            with open(in_bam, "rb") as f:
                tail = np.zeros(0, dtype=np.uint8)
                while True:
                    t1 = time.perf_counter()
                    raw = np.fromfile(f, dtype=np.uint8, count=int(segment_bytes))
                    last = raw.size < int(segment_bytes)
                    comp = np.concatenate([tail, raw]) if tail.size else raw
                    buf, used = _lib.bgzf_inflate(comp, n_threads=n_threads) if comp.size else (np.zeros(0, dtype=np.uint8), 0)
                    tail = comp[used:].copy()
                    if last and tail.size:
                        raise _lib.SmiError(f"{in_bam}: truncated BGZF stream")
                    segments.put((buf, last, None, time.perf_counter() - t1))
                    if last:
                        return
        except BaseException as e:  # noqa: BLE001 -- handed to the consumer
            segments.put((None, True, e, 0.0))

    try:
        threading.Thread(target=reader, daemon=True).start()
        pend = np.zeros(0, dtype=np.uint8)
        header = False
        eof = False
        while not eof:
            buf, eof, e, dt = segments.get()
            if e is not None:
                raise e
            secs["bam_read_inflate"] += dt
            bam = np.concatenate([pend, buf]) if pend.size else buf
            start = 0
            if not header:
                try:
                    _text, _refs, start = _lib.bam_header(bam)
                except _lib.SmiError:
                    if eof:
                        raise
                    pend = bam                    # the header is not complete yet: read on
                    continue
                header = True
            t1 = time.perf_counter()
            recs, end = _lib.bam_index_records(bam, start, cap=max(1, (bam.size - start) // 36))
            if eof and end != bam.size:
                raise _lib.SmiError(f"{in_bam}: truncated BAM record")
            secs["index"] += time.perf_counter() - t1
            t1 = time.perf_counter()
            if recs.size:
                h.add_segment(bam, recs)
            secs["parse"] += time.perf_counter() - t1
            pend = bam[end:].copy()
        if not header:
            raise _lib.SmiError(f"{in_bam}: no BAM header")
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
