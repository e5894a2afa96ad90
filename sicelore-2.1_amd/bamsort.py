"""`BamSort`: the coordinate sort of a BAM, with its `.bai` on request, where the reference's scripts say `samtools sort x.bam -o y.bam`
and `samtools index y.bam` (quickrun-2.1.step4b.sh:53-54, the tail of every mapping line).

    python sicelore-2.1_amd/bamsort.py [-@ N] [-m MEM] [-T PREFIX] [-l LEVEL] [--resident-bytes N] [--write-index] -o out.bam in.bam

-m and -l are read and have no effect: what stays resident follows from the device memory, and the deflater has one level.  -T PREFIX is
the prefix of the temporary files, as in samtools (without it <out.bam>.tmp<pid>): a BAM that does not fit the device is sorted through
run files PREFIX.0000.run, PREFIX.0001.run, ... of raw records, as large as the inflated file together, and a merge; they are removed at
the end, whatever the end is, and where the file fits none is written.  --resident-bytes N bounds the device memory the records take
(default: two fifths of what is free); the file is then read in segments of at most N / 32 compressed bytes, since a run ends where a
segment ends.  -n, -t, -M, -O with anything but bam, a missing -o, `-` as input and more than one input are
refused.  It has a command line of its own: `samtools` is not a `java` line, so `cli.main`, `python sicelore-2.1_amd` and `bin/java` do
not know it.

The BAM is read in segments (bamsegments.segments); the record bytes of every segment stay in one device arena, K-SORT-KEY
(smi_bamsort.hip) gives every record its key, one stable radix sort orders them, and the output leaves in windows: K-SORT-GATHER copies
the records of a window in rank order, the library's deflater makes its BGZF blocks.  The order is this build's own canonical definition
(DESIGN.md section 8m): the reference rank (records without a reference last), pos + 1 as an unsigned number, forward before reverse;
equal keys keep their input order.  No byte equality with `samtools sort` is claimed.  The header's @HD line gets SO:coordinate; no @PG
line is added.  A ref_id outside the header raises lib.BamSortError, which names the read and its 0-based number; sort_bam without
runs_prefix refuses a BAM that does not fit the device by name, and so is a single segment that does not fit (lower segment_bytes);
nothing is left on disk in any of these cases.  At most 2^31 - 1 records.  The output goes to a temporary file beside it that takes its name
at the end."""
import os
import struct
import sys
import time

if __name__ == "__main__" and "sicelore_amd" not in sys.modules:      # run as a file: the package under the name the repository uses for it
    import importlib.util
    _HERE = os.path.dirname(os.path.abspath(__file__))
    _spec = importlib.util.spec_from_file_location("sicelore_amd", os.path.join(_HERE, "__init__.py"), submodule_search_locations=[_HERE])
    _mod = importlib.util.module_from_spec(_spec)
    sys.modules["sicelore_amd"] = _mod
    _spec.loader.exec_module(_mod)
    from sicelore_amd import bamsort as _self
    sys.exit(_self.main())

import numpy as np

from . import lib as _lib
from .bamsegments import BGZF_EOF, segments


def sorted_header(hdr):
    """the header's bytes (magic, l_text, text, reference dictionary) with SO:coordinate: an @HD line in front has its SO: field set, or
    appended where it has none, its other fields as they are; a text without one gets `@HD VN:1.6 SO:coordinate` in front"""
    hdr = bytes(hdr)
    l_text = struct.unpack_from("<I", hdr, 4)[0]
    text, rest = hdr[8:8 + l_text], hdr[8 + l_text:]
    line, nl, after = text.partition(b"\n")
    fields = line.split(b"\t")
    if fields[0] == b"@HD":
        at = [k for k, f in enumerate(fields) if k and f.startswith(b"SO:")]
        if at:
            fields[at[0]] = b"SO:coordinate"
        else:
            fields.append(b"SO:coordinate")
        text = b"\t".join(fields) + nl + after
    else:
        text = b"@HD\tVN:1.6\tSO:coordinate\n" + text
    return hdr[:4] + struct.pack("<I", len(text)) + text + rest


def sort_bam(ctx, in_bam, out_bam, index=False, segment_bytes=256 << 20, window_bytes=64 << 20, resident_bytes=None, n_threads=4, runs_prefix=None):
    """-> dict of counts (records, segments, windows, arena_bytes, runs, ...), device ms per stage, seconds, bytes written and wall time.
    index: also leave <out_bam>.bai, built from the records and the BGZF blocks as they are written (bamindex.WriterIndex); the info then
    has `index` (its counts and times; None where no index can be built over the sorted file: the BAM is kept and `index_error` says why).
    resident_bytes: the bound on the device memory the records take (None: from the free device memory).
    runs_prefix: None refuses a BAM beyond resident_bytes.  With a string such a BAM is sorted through run files
    "<runs_prefix>.<%04d>.run", one per arena-full, each the raw records of the run in sorted order (as large as the inflated file together),
    and a merge that reads one slice of every run per output window; the written BAM is the same file, byte for byte.  Where everything
    fits no run file is created.  Every run file is removed on every way out.  At most 2^31 - 1 records either way."""
    t_all = time.perf_counter()
    tmp = f"{out_bam}.tmp{os.getpid()}"
    secs = dict(bam_read_inflate=0.0, index=0.0, device=0.0, write=0.0)
    stage_ms = dict.fromkeys(_lib.BAMSORT_STAGES, 0.0)
    h = wix = None
    written = 0
    run_paths, run_fds = [], []

    def timed(call, *args, **kw):
        t0 = time.perf_counter()
        out = call(*args, **kw)
        secs["device"] += time.perf_counter() - t0
        for k, v in h.stage_ms().items():
            stage_ms[k] += v
        return out

    def spill():
        """what the arena holds becomes the next run file: its windows as they come, raw"""
        n_run_windows, _n, _bytes = timed(h.spill_begin)
        run_paths.append(f"{runs_prefix}.{len(run_paths):04d}.run")
        with open(run_paths[-1], "wb") as f:
            for k in range(n_run_windows):
                data = timed(h.spill_window, k)
                t0 = time.perf_counter()
                f.write(memoryview(data))
                secs["run_write"] = secs.get("run_write", 0.0) + time.perf_counter() - t0
        timed(h.spill_end)

    def slices_of(k, buf):
        """the slice of every run file that window k draws, one behind the other in run order -> the filled part of buf"""
        first, size, _ordinal = h.window_slices(k)
        t0 = time.perf_counter()
        view, at = memoryview(buf), 0
        for fd, off, n in zip(run_fds, first.tolist(), size.tolist()):
            end = at + n
            while at < end:
                got = os.preadv(fd, [view[at:end]], off)
                if got <= 0:
                    raise _lib.SmiError(f"{runs_prefix}: a run file ends inside a slice of window {k}")
                at, off = at + got, off + got
        secs["run_read"] = secs.get("run_read", 0.0) + time.perf_counter() - t0
        return buf[:at]

    try:
        header = None
        for bam, recs, hdr in segments(in_bam, segment_bytes, n_threads, secs):
            if hdr is not None:
                _text, refs, _start = _lib.bam_header(np.frombuffer(hdr, dtype=np.uint8))
                header = sorted_header(hdr)
                h = _lib.BamSort(ctx, len(refs), resident_bytes, window_bytes)
                if runs_prefix is not None:
                    h.run_mode()
            if recs.size and not timed(h.add_segment, bam, recs):
                spill()                                   # full: the arena becomes a run, the segment goes into the empty arena
                if not timed(h.add_segment, bam, recs):   # (cannot happen: a segment beyond the empty arena is refused by name)
                    raise _lib.SmiError("BamSort: a segment does not fit the empty arena")
        if run_paths:
            spill()                                       # uniform: the last arena-full is a run like the others
        n_windows, _n_records = timed(h.finish)
        slices = None
        if run_paths:
            run_fds.extend(os.open(p, os.O_RDONLY) for p in run_paths)
            slices = np.empty(max(h.counts()["largest_window"], 1), dtype=np.uint8)
        if index:
            from .bamindex import WriterIndex
            wix = WriterIndex(ctx)
        with open(tmp, "wb") as f:
            t0 = time.perf_counter()
            z = ctx.bgzf_deflate_device(np.frombuffer(header, dtype=np.uint8))[:-len(BGZF_EOF)]
            secs["device"] += time.perf_counter() - t0
            f.write(memoryview(z))
            if wix is not None:
                wix.emitted(header, z, written, records=False)
            written += len(z)
            for k in range(n_windows):
                if run_paths:
                    z, data = timed(h.merge_window, k, slices_of(k, slices), inflated=index)
                else:
                    z, data = timed(h.window, k, inflated=index)
                t0 = time.perf_counter()
                f.write(memoryview(z))
                secs["write"] += time.perf_counter() - t0
                if wix is not None:
                    wix.emitted(data, z, written)
                written += len(z)
            f.write(BGZF_EOF)
            written += len(BGZF_EOF)
        os.replace(tmp, out_bam)
        if not run_paths:                                 # the stages of the runs are named where there were runs
            stage_ms = {k: v for k, v in stage_ms.items() if k not in _lib.BAMSORT_RUN_STAGES}
        info = dict(h.counts(), stage_ms=stage_ms, seconds=secs, bytes_written=written, windows=n_windows)
        if wix is not None:
            info["index"], info["index_error"] = wix.finish(f"{out_bam}.bai", written - len(BGZF_EOF))
    finally:
        if wix is not None:
            wix.close()
        if h is not None:
            h.close()
        for fd in run_fds:
            os.close(fd)
        for p in run_paths + [tmp]:
            if os.path.exists(p):
                os.remove(p)
    info["wall_s"] = time.perf_counter() - t_all
    return info


USAGE = "usage: bamsort.py [-@ N] [-m MEM] [-T PREFIX] [-l LEVEL] [--resident-bytes N] [--write-index] -o out.bam in.bam"
NO_EFFECT = {"-m": "what stays resident follows from the device memory", "-l": "the deflater has one level"}
REFUSED = {"-n": "a sort by read name is not built", "-t": "a sort by tag is not built", "-M": "the minimiser order is not built"}


def main(argv=None):
    """-> exit code: 0, or 1 with the message on stderr (argument errors, and the record the sort stops at, named)"""
    from . import cli
    argv = list(sys.argv[1:] if argv is None else argv)
    try:
        if not argv or argv[0] in ("-h", "--help", "help"):
            print(__doc__)
            return 0
        threads = out_bam = fmt = prefix = resident = None
        write_index, paths = False, []
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
            elif a == "-T":
                prefix, k = value(a, k), k + 2
            elif a.startswith("-T") and len(a) > 2:
                prefix, k = a[2:], k + 1
            elif a == "--resident-bytes":
                resident, k = value(a, k), k + 2
            elif a in NO_EFFECT:                       # read, no effect
                value(a, k)
                k += 2
            elif a[:2] in NO_EFFECT and len(a) > 2:
                k += 1
            elif a == "--write-index":
                write_index, k = True, k + 1
            elif a in REFUSED or (a[:2] == "-t" and len(a) > 2):
                raise cli.CliError(f"{a[:2]}: {REFUSED[a[:2]]} in this build: bamsort.py sorts by coordinate")
            elif a == "-":
                raise cli.CliError("-: the input is a file in this build, not the standard input")
            elif a.startswith("-") and len(a) > 1:
                raise cli.CliError(f"unknown option {a!r}; {USAGE}")
            else:
                paths.append(a)
                k += 1
        if fmt is not None and fmt.lower() != "bam":
            raise cli.CliError(f"-O {fmt}: this build writes BAM alone")
        if threads is not None:
            try:
                threads = int(threads)
            except ValueError:
                raise cli.CliError(f"-@ {threads!r}: not a number")
            if threads < 0:
                raise cli.CliError(f"-@ {threads}: not a thread count")
        if resident is not None:
            try:
                resident = int(resident)
            except ValueError:
                raise cli.CliError(f"--resident-bytes {resident!r}: not a number")
            if resident <= 0:
                raise cli.CliError(f"--resident-bytes {resident}: not a number of bytes")
        if out_bam is None:
            raise cli.CliError(f"-o is missing: this build writes a file, not the standard output; {USAGE}")
        if len(paths) > 1:
            raise cli.CliError(f"more than one input ({', '.join(paths)}): this build sorts one BAM; {USAGE}")
        if not paths:
            raise cli.CliError(USAGE)
        in_bam = paths[0]
        if not os.path.isfile(in_bam):
            raise cli.CliError(f"{in_bam}: no such file")
        if not os.path.isdir(os.path.dirname(os.path.abspath(out_bam))) or os.path.isdir(out_bam):
            raise cli.CliError(f"{out_bam}: no such directory, or a directory")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise cli.CliError("bamsort.py runs in one process on one GPU in this build: start it without torchrun")
        n_threads = max(1, min(threads, 16)) if threads else cli._ncpu({})       # samtools' -@ counts additional threads; 0 = none
        try:
            # the prefix's directory is looked at when a run is written: a file that fits needs none.  A run is cut at a segment border,
            # so under a given budget the reader's segments (compressed bytes) are small enough for several to fit one
            sizes = {} if resident is None else dict(segment_bytes=min(256 << 20, max(1 << 10, resident // 32)))
            info = sort_bam(cli._context(), in_bam, out_bam, index=write_index, n_threads=n_threads, resident_bytes=resident,
                            runs_prefix=prefix if prefix is not None else f"{out_bam}.tmp{os.getpid()}", **sizes)
        except _lib.BamSortError as e:
            raise cli.CliError(f"{in_bam}: {e}; {out_bam} was not written")
        runs = f", through {info['runs']} runs of {info['run_bytes']} bytes" if info.get("runs") else ""
        print(f"DONE -- {info['records']} records in {info['segments']} segments, {info['windows']} windows, {info['bytes_written']} bytes written{runs}",
              file=sys.stderr)
        if info.get("index_error"):
            print(f"WARNING: {info['index_error']}", file=sys.stderr)
        return 0
    except cli.CliError as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return 1
    except (_lib.SmiError, OSError, ValueError) as e:
        print(f"ERROR: {type(e).__name__}: {e}", file=sys.stderr)
        return 1
