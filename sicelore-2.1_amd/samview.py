"""`SamView`: SAM text to BAM, where the reference's scripts say `samtools view -bS x.sam -o x.bam` (quickrun-2.1.step4b.sh:52, in front
of every `samtools sort`).

    python sicelore-2.1_amd/samview.py [-b] [-S] [-h] [-@ N] -o out.bam in.sam|-

-S and -h are read and have no effect: the input is SAM text and the header is always written.  Flags may stand in one cluster (-bS, -Sb)
and -o may stand behind the input.  A missing -b, a missing -o, a region behind the input, BAM input, -O with anything but bam, and
-f -F -q -L -r -R -s -c -1 -u are refused.  It has a command line of its own: `samtools` is not a `java` line, so `cli.main`,
`python sicelore-2.1_amd` and `bin/java` do not know it.

The text is read in segments that end on a line end (`-` reads the standard input the same way); the header lines become the BAM header
on the host, K-SAM-SIZE and K-SAM-WRITE (smi_samview.hip) turn the alignment lines of a segment into records, the library's deflater makes
their BGZF blocks.  The conversion is this build's own canonical definition; no byte equality with `samtools view`
is claimed.  No @PG line is added.  A line that breaks a rule raises lib.SamViewError, which names its 1-based number in the file and the
rule; nothing is written then.  The output goes to a temporary file beside it that takes its name at the end."""
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
    from sicelore_amd import samview as _self
    sys.exit(_self.main())

import numpy as np

from . import lib as _lib
from .bamsegments import BGZF_EOF

MAX_LINE = 1 << 30


def text_segments(f, segment_bytes, secs=None):
    """f: a binary stream of SAM text -> first the header (the leading @ lines as they stand, bytes), then the alignment lines in pieces
    of about segment_bytes that begin at a line's start and end behind an LF (the last one at the end of the input).  A line longer than
    a segment grows the piece."""
    def read(n):
        t0 = time.perf_counter()
        b = f.read(n)
        if secs is not None:
            secs["read"] += time.perf_counter() - t0
        return b

    buf, eof = bytearray(), False

    def more():
        nonlocal eof
        b = read(segment_bytes)
        if not b:
            eof = True
        buf.extend(b)
        if len(buf) > MAX_LINE + segment_bytes:
            raise _lib.SmiError("SamView: a line of more than 2^30 bytes")

    at = 0                                              # the header: while the line at `at` begins with @
    while True:
        if at == len(buf) and not eof:
            more()
            continue
        if at < len(buf) and buf[at] == 64:
            nl = buf.find(b"\n", at)
            if nl < 0 and not eof:
                more()
                continue
            at = len(buf) if nl < 0 else nl + 1
            continue
        break
    yield bytes(buf[:at])
    del buf[:at]
    while True:
        while len(buf) < segment_bytes and not eof:
            more()
        if not buf:                                     # (the end of the input)
            return
        cut = len(buf) if eof else buf.rfind(b"\n") + 1
        if not cut:                                     # no LF yet: the line goes on
            more()
            continue
        piece = np.frombuffer(bytes(buf[:cut]), dtype=np.uint8)
        del buf[:cut]
        yield piece


def sam_to_bam(ctx, in_sam, out_bam, index=False, segment_bytes=256 << 20, n_threads=4):
    """-> dict of counts (records, segments, text_bytes, record_bytes, references), device ms per stage, seconds, bytes written and wall
    time.  in_sam: a path, `-` (the standard input) or a binary stream.  index: also leave <out_bam>.bai, built from the records and the
    BGZF blocks as they are written (bamindex.WriterIndex); the info then has `index` (None where no index can be built, which is the
    normal case for the unsorted output of a mapper: the BAM is kept and `index_error` says why).  n_threads: read for the command
    line's -@; the text is read on one thread."""
    t_all = time.perf_counter()
    tmp = f"{out_bam}.tmp{os.getpid()}"
    secs = dict(read=0.0, device=0.0, write=0.0)
    stage_ms = dict.fromkeys(_lib.SAMVIEW_STAGES, 0.0)
    h = wix = None
    written = 0
    src = sys.stdin.buffer if in_sam == "-" else open(in_sam, "rb") if isinstance(in_sam, (str, os.PathLike)) else in_sam

    def timed(call, *args, **kw):
        t0 = time.perf_counter()
        out = call(*args, **kw)
        secs["device"] += time.perf_counter() - t0
        return out

    try:
        pieces = text_segments(src, int(segment_bytes), secs)
        h = timed(_lib.SamView, ctx, next(pieces))
        header = h.header()
        if index:
            from .bamindex import WriterIndex
            wix = WriterIndex(ctx)
        with open(tmp, "wb") as f:
            z = timed(ctx.bgzf_deflate_device, np.frombuffer(header, dtype=np.uint8))[:-len(BGZF_EOF)]
            f.write(memoryview(z))
            if wix is not None:
                wix.emitted(header, z, written, records=False)
            written += len(z)
            for piece in pieces:
                timed(h.add_segment, piece)
                z, data = timed(h.convert, inflated=index)
                for k, v in h.stage_ms().items():
                    stage_ms[k] += v
                t0 = time.perf_counter()
                f.write(memoryview(z))
                secs["write"] += time.perf_counter() - t0
                if wix is not None:
                    wix.emitted(data, z, written)
                written += len(z)
            f.write(BGZF_EOF)
            written += len(BGZF_EOF)
        os.replace(tmp, out_bam)
        info = dict(h.counts(), stage_ms=stage_ms, seconds=secs, bytes_written=written)
        if wix is not None:
            info["index"], info["index_error"] = wix.finish(f"{out_bam}.bai", written - len(BGZF_EOF))
    finally:
        if wix is not None:
            wix.close()
        if h is not None:
            h.close()
        if src is not in_sam and src is not sys.stdin.buffer:
            src.close()
        if os.path.exists(tmp):
            os.remove(tmp)
    info["wall_s"] = time.perf_counter() - t_all
    return info


USAGE = "usage: samview.py [-b] [-S] [-h] [-@ N] -o out.bam in.sam|-"
NO_EFFECT = {"S": "the input is SAM text", "h": "the header is always written"}
REFUSED = {"f": "a filter on flag bits", "F": "a filter on flag bits", "q": "a filter on MAPQ", "L": "a filter on a BED file", "r": "a filter on read groups",
           "R": "a filter on read groups", "s": "subsampling", "c": "counting", "1": "the fast compression level", "u": "uncompressed output"}
BAM_MAGIC = b"\x1f\x8b"


def main(argv=None):
    """-> exit code: 0, or 1 with the message on stderr (argument errors, and the line the conversion stops at, named)"""
    from . import cli
    argv = list(sys.argv[1:] if argv is None else argv)
    try:
        if not argv or argv[0] in ("--help", "help"):
            print(__doc__)
            return 0
        threads = out_bam = fmt = None
        binary, paths = False, []
        k = 0

        def value(a, k):
            if k + 1 >= len(argv):
                raise cli.CliError(f"{a} needs a value; {USAGE}")
            return argv[k + 1]

        while k < len(argv):
            a = argv[k]
            if a == "-@" or a == "--threads":
                threads, k = value(a, k), k + 2
            elif a.startswith("-@") and len(a) > 2:
                threads, k = a[2:], k + 1
            elif a == "-o":
                out_bam, k = value(a, k), k + 2
            elif a == "-O" or a == "--output-fmt":
                fmt, k = value(a, k), k + 2
            elif a == "-":
                paths.append(a)
                k += 1
            elif a.startswith("-") and not a.startswith("--"):          # a cluster of flags
                for c in a[1:]:
                    if c == "b":
                        binary = True
                    elif c in REFUSED:
                        raise cli.CliError(f"-{c}: {REFUSED[c]} is not built: samview.py converts every line of SAM text to BAM")
                    elif c not in NO_EFFECT:
                        raise cli.CliError(f"unknown option {a!r}; {USAGE}")
                k += 1
            elif a.startswith("--"):
                raise cli.CliError(f"unknown option {a!r}; {USAGE}")
            else:
                paths.append(a)
                k += 1
        if fmt is not None and fmt.lower() != "bam":
            raise cli.CliError(f"-O {fmt}: this build writes BAM alone")
        if not binary and fmt is None:
            raise cli.CliError(f"-b is missing: this build writes BAM alone; {USAGE}")
        if threads is not None:
            try:
                threads = int(threads)
            except ValueError:
                raise cli.CliError(f"-@ {threads!r}: not a number")
            if threads < 0:
                raise cli.CliError(f"-@ {threads}: not a thread count")
        if out_bam is None:
            raise cli.CliError(f"-o is missing: this build writes a file, not the standard output; {USAGE}")
        if not paths:
            raise cli.CliError(USAGE)
        if len(paths) > 1:
            raise cli.CliError(f"{' '.join(paths[1:])}: a region behind the input is not built: samview.py converts the whole text; {USAGE}")
        in_sam = paths[0]
        if in_sam != "-":
            if not os.path.isfile(in_sam):
                raise cli.CliError(f"{in_sam}: no such file")
            with open(in_sam, "rb") as f:
                if f.read(2) == BAM_MAGIC:
                    raise cli.CliError(f"{in_sam}: BAM or gzip input: this build reads SAM text")
        if not os.path.isdir(os.path.dirname(os.path.abspath(out_bam))) or os.path.isdir(out_bam):
            raise cli.CliError(f"{out_bam}: no such directory, or a directory")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise cli.CliError("samview.py runs in one process on one GPU in this build: start it without torchrun")
        n_threads = max(1, min(threads, 16)) if threads else cli._ncpu({})       # samtools' -@ counts additional threads; 0 = none
        try:
            info = sam_to_bam(cli._context(), in_sam, out_bam, n_threads=n_threads)
        except _lib.SamViewError as e:
            raise cli.CliError(f"{in_sam}: {e}; {out_bam} was not written")
        print(f"DONE -- {info['records']} records in {info['segments']} segments, {info['bytes_written']} bytes written", file=sys.stderr)
        return 0
    except cli.CliError as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return 1
    except (_lib.SmiError, OSError, ValueError) as e:
        print(f"ERROR: {type(e).__name__}: {e}", file=sys.stderr)
        return 1
