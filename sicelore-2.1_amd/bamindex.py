"""`BamIndex`: the `.bai` (SAM specification 5.2) of a coordinate-sorted BAM, where the reference's scripts say `samtools index`
(quickrun-2.1.sh, sicelore-nf/main.nf:117 and after AddBamMoleculeTags, AddGeneNameTag and IsoformMatrix ISOBAM=true).

    python sicelore-2.1_amd/bamindex.py [-@ N] in.bam [out.bai]          # samtools index [-@ N] in.bam [out.bai]

It has a command line of its own: `samtools` is not a `java` line, so `cli.main`, `python sicelore-2.1_amd` and `bin/java` do not know it.

The BAM is read in segments (bamsegments.segments) that come with the table of their BGZF blocks; K-BAI (smi_bamindex.hip) gives every
record its extent, bin, windows and virtual offsets, checks the order, compacts the runs of one bin into chunks and fills the linear
index; at the end one sort by (reference, bin) and the host writes the file.  The index is this build's own canonical form (DESIGN.md
section 8l): every reader of the format reads it, and it is not byte-equal to the file of samtools or of htsjdk.  A record out of
coordinate order, one on a reference with a negative position and one that ends behind 2^29 raise lib.BamIndexError, which names the
read and its 0-based number; nothing is written then.  The index goes to a temporary file beside the output that takes the output's name
at the end."""
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
    from sicelore_amd import bamindex as _self
    sys.exit(_self.main())

import numpy as np

from . import lib as _lib
from .bamsegments import segments


class Indexer:
    """A lib.BamIndex fed as a writer or a reader goes: header(bytes) creates the handle from the reference dictionary, blocks(...) takes
    the next BGZF blocks (kept until the handle exists), segment(bam, recs, stream_off) a segment, finish() -> the .bai's bytes."""

    def __init__(self, ctx):
        self._ctx, self.h, self._wait = ctx, None, []
        self.stage_ms = dict.fromkeys(_lib.BAMINDEX_STAGES, 0.0)
        self.device_s = 0.0

    def header(self, hdr):
        _text, refs, _start = _lib.bam_header(np.frombuffer(hdr, dtype=np.uint8))
        self.h = _lib.BamIndex(self._ctx, [r[1] for r in refs])

    def blocks(self, coffset, isize, end_coffset):
        self._wait.append((coffset, isize, end_coffset))

    def _flush(self):
        for b in self._wait:
            self.h.add_blocks(*b)
        self._wait = []

    def _timed(self, call, *args):
        t0 = time.perf_counter()
        out = call(*args)
        self.device_s += time.perf_counter() - t0
        for k, v in self.h.stage_ms().items():
            self.stage_ms[k] += v
        return out

    def segment(self, bam, recs, stream_off):
        self._flush()
        self._timed(self.h.add_segment, bam, recs, stream_off)

    def finish(self):
        self._flush()
        return self._timed(self.h.finish)

    def close(self):
        if self.h is not None:
            self.h.close()


class WriterIndex:
    """The index as a by-product of a BAM writer, which holds every record it writes, inflated, and the BGZF blocks it deflated them into.
    emitted() after every piece written, finish() once the BAM has its final name.  A record no index can be built over ends the index
    and not the writer: the BAM is kept, no .bai is written, and finish() says why."""

    def __init__(self, ctx):
        self.ix, self.stream, self.error = Indexer(ctx), 0, None
        self.seconds = 0.0

    def emitted(self, data, z, coffset, records=True):
        """data: the inflated bytes (the whole header with records=False, else whole alignment records), z: the BGZF blocks they were
        deflated into, written at file offset coffset"""
        if self.error is not None:
            return
        t0 = time.perf_counter()
        data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data
        try:
            if not records:
                self.ix.header(data)
            coff, isize, used = _lib.bgzf_block_table(z, base=coffset)
            self.ix.blocks(coff, isize, coffset + used)
            if records and data.size:
                recs, end = _lib.bam_index_records(data, 0, cap=max(1, data.size // 36))
                if end != data.size:
                    raise _lib.SmiError("BamIndex: the bytes written do not end with a whole record")
                self.ix.segment(data, recs, self.stream)
        except _lib.BamIndexError as e:
            self.error = e
        self.stream += data.size
        self.seconds += time.perf_counter() - t0

    def finish(self, out_bai, eof_coffset, log=None):
        """eof_coffset: where the writer put the end-of-file block -> (info of the index or None, the reason it was not written or None)"""
        try:
            if self.error is not None:
                why = f"{self.error}; the BAM is complete, {out_bai} was not written"
                if log is not None:
                    print(f"WARNING: {why}", file=log)
                return None, why
            t0 = time.perf_counter()
            self.ix.blocks([eof_coffset], [0], eof_coffset + 28)
            data = self.ix.finish()
            written = write_bai(out_bai, data)
            self.seconds += time.perf_counter() - t0
            return dict(self.ix.h.counts(), path=out_bai, stage_ms=self.ix.stage_ms, seconds=self.seconds, bytes_written=written), None
        finally:
            self.ix.close()

    def close(self):
        self.ix.close()


def write_bai(out_bai, data):
    """data under the name out_bai, through a temporary file beside it -> bytes written"""
    tmp = f"{out_bai}.tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            f.write(data)
        os.replace(tmp, out_bai)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return len(data)


def index_bam(ctx, in_bam, out_bai=None, segment_bytes=256 << 20, n_threads=4):
    """-> dict of counts (records, refs_with_records, chunks, no_coor, ...), device ms per stage, seconds, bytes written and wall time.
    out_bai: default <in_bam>.bai."""
    t_all = time.perf_counter()
    out_bai = f"{in_bam}.bai" if out_bai is None else out_bai
    secs = dict(bam_read_inflate=0.0, index=0.0, device=0.0, write=0.0)
    ix = Indexer(ctx)
    offs = []

    def on_blocks(coffset, isize, end_coffset, stream_off):
        ix.blocks(coffset, isize, end_coffset)
        offs.append(stream_off)

    try:
        for bam, recs, hdr in segments(in_bam, segment_bytes, n_threads, secs, blocks=on_blocks):
            if hdr is not None:
                ix.header(hdr)
            if recs.size:
                ix.segment(bam, recs, offs[-1])
        data = ix.finish()
        counts = ix.h.counts()
        t0 = time.perf_counter()
        written = write_bai(out_bai, data)
        secs["write"] = time.perf_counter() - t0
    finally:
        ix.close()
    secs["device"] = ix.device_s
    return dict(counts, stage_ms=ix.stage_ms, seconds=secs, bytes_written=written, wall_s=time.perf_counter() - t_all)


USAGE = "usage: bamindex.py [-@ N] in.bam [out.bai]"


def main(argv=None):
    """-> exit code: 0, or 1 with the message on stderr (argument errors, and the records no index can be built over, named)"""
    from . import cli
    argv = list(sys.argv[1:] if argv is None else argv)
    try:
        if not argv or argv[0] in ("-h", "--help", "help"):
            print(__doc__)
            return 0
        threads, paths = None, []
        k = 0
        while k < len(argv):
            a = argv[k]
            if a == "-@" or a == "--threads":
                if k + 1 >= len(argv):
                    raise cli.CliError(f"{a} needs a number; {USAGE}")
                threads, k = argv[k + 1], k + 2
            elif a.startswith("-@") and len(a) > 2:
                threads, k = a[2:], k + 1
            elif a.startswith("-") and len(a) > 1:
                raise cli.CliError(f"unknown option {a!r}; {USAGE}")
            else:
                paths.append(a)
                k += 1
        if threads is not None:
            try:
                threads = int(threads)
            except ValueError:
                raise cli.CliError(f"-@ {threads!r}: not a number")
            if threads < 0:
                raise cli.CliError(f"-@ {threads}: not a thread count")
        if not 1 <= len(paths) <= 2:
            raise cli.CliError(USAGE)
        in_bam = paths[0]
        out_bai = paths[1] if len(paths) == 2 else f"{in_bam}.bai"
        if not os.path.isfile(in_bam):
            raise cli.CliError(f"{in_bam}: no such file")
        if not os.path.isdir(os.path.dirname(os.path.abspath(out_bai))) or os.path.isdir(out_bai):
            raise cli.CliError(f"{out_bai}: no such directory, or a directory")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise cli.CliError("bamindex.py runs in one process on one GPU in this build: start it without torchrun")
        n_threads = max(1, min(threads, 16)) if threads else cli._ncpu({})       # samtools' -@ counts additional threads; 0 = none
        try:
            info = index_bam(cli._context(), in_bam, out_bai, n_threads=n_threads)
        except _lib.BamIndexError as e:
            raise cli.CliError(f"{in_bam}: {e}; {out_bai} was not written")
        print(f"DONE -- {info['records']} records, {info['refs_with_records']} references with records, {info['chunks']} chunks, "
              f"{info['no_coor']} records without a reference", file=sys.stderr)
        return 0
    except cli.CliError as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return 1
    except (_lib.SmiError, OSError, ValueError) as e:
        print(f"ERROR: {type(e).__name__}: {e}", file=sys.stderr)
        return 1
