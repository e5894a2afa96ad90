"""`BamView`: region and flag queries of an indexed BAM, where the reference's scripts say `samtools view` with a BAM as its input
(sicelore-nf/main.nf:129 `samtools view -H $bam`, the list of chromosomes, and main.nf:143 `samtools view -Sb $bam $chromo -o
chromosome.bam`, the split that feeds ComputeConsensus one chromosome at a time).

    python sicelore-2.1_amd/bamview.py [-b] [-S] [-h] [-@ N] [-f INT] [-F INT] [-q INT] [--write-index] -o out.bam in.bam [region ...]
    python sicelore-2.1_amd/bamview.py -H in.bam                       # the header text, to the standard output (or to -o)
    python sicelore-2.1_amd/bamview.py -c [-f INT] [-F INT] [-q INT] in.bam [region ...]          # the number of kept records

-S and -h are read and have no effect.  Flags may stand in one cluster (-Sb) and -o may stand anywhere, so main.nf:143's argument order
parses as it stands.  -f and -F take decimal or 0x hexadecimal numbers.  A missing -b without -H or -c, a missing -o where a BAM is
written, SAM text or `-` as input, -O with anything but bam, and -L -r -R -s -d -D -1 -u -U -M -X are refused.  It has a command line of
its own: `samtools` is not a `java` line, so `cli.main`, `python sicelore-2.1_amd` and `bin/java` do not know it; samview.py keeps
refusing BAM input.

A region is NAME, NAME:BEG or NAME:BEG-END, 1-based and inclusive, commas allowed in the numbers; a text that is a reference name as a
whole is that reference, any other text is split at its last colon.  With regions the index (<in>.bai, else <in without .bam>.bai) is read
as the specification describes (SAM 5.3), so `samtools`' and htsjdk's files are read as well as bamindex.py's: the chunks of the bins a
region may touch, cut by the linear index, merged over all regions into ranges of virtual offsets; only the BGZF blocks under the ranges
are read and inflated (bamsegments.ranges).  Without regions the file is streamed (bamsegments.segments).  K-VIEW-TEST
(smi_bamview.hip) gives every record its extent from the stored CIGAR and tests the filters and the merged regions, a scan gives the
kept records their places, K-VIEW-GATHER copies them, the library's deflater makes their BGZF blocks.  The definition is DESIGN.md
section 8o; no byte equality with `samtools view` is claimed.  The header is the input's; no @PG line is added.  A ref_id outside the
header raises lib.BamViewError, a missing index, one with another number of references and one whose chunks are not this file's records
raise ViewStop; nothing is left on disk then.  The output goes to a temporary file beside it that takes its name at the end."""
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
    from sicelore_amd import bamview as _self
    sys.exit(_self.main())

import numpy as np

from . import bamsegments
from . import lib as _lib
from .bamsegments import BGZF_EOF

MAX_END = 1 << 29          # the last position the bins and the 16 kb windows of a .bai hold
META_BIN = 37450
LEVELS = ((0, 29), (1, 26), (9, 23), (73, 20), (585, 17), (4681, 14))          # (first bin, log2 of the bin's width)


class ViewStop(_lib.SmiError):
    """the run stops before anything is written: a region that names nothing, a missing index, an index that is not the file's"""


# ---- regions ------------------------------------------------------------------------------------------------------------------------------
def _number(text, part):
    digits = part.replace(",", "")
    if not digits or not digits.isascii() or not digits.isdigit():
        raise ViewStop(f"region {text!r}: {part!r} is not a number (decimal digits, commas allowed)")
    return int(digits)


def parse_region(text, ref_names):
    """NAME, NAME:BEG or NAME:BEG-END (1-based, inclusive) -> (ref_id, beg, end), 0-based and half-open.  A text that is a reference name
    as a whole is that reference even if it holds a colon; any other text is split at its last colon.  A missing END is 2^29, a given one
    is capped there.  A name that occurs twice means its first entry."""
    names = list(ref_names)
    if text in names:
        return names.index(text), 0, MAX_END
    name, colon, span = text.rpartition(":")
    if not colon or name not in names:
        raise ViewStop(f"region {text!r}: {name if colon else text!r} is not one of the header's references")
    first, dash, last = span.partition("-")
    beg = _number(text, first)
    end = _number(text, last) if dash else None
    if beg < 1:
        raise ViewStop(f"region {text!r}: BEG is below 1")
    if end is not None and end < beg:
        raise ViewStop(f"region {text!r}: END is below BEG")
    return names.index(name), beg - 1, MAX_END if end is None else min(end, MAX_END)


def resolve_regions(regions, ref_names):
    """texts and (name or ref_id, beg0, end0) tuples -> [(ref_id, beg, end)]"""
    names = list(ref_names)
    out = []
    for r in regions:
        if isinstance(r, str):
            out.append(parse_region(r, names))
            continue
        ref, beg, end = r
        if isinstance(ref, str):
            if ref not in names:
                raise ViewStop(f"region {r!r}: {ref!r} is not one of the header's references")
            ref = names.index(ref)
        ref, beg, end = int(ref), int(beg), int(end)
        if not 0 <= ref < len(names):
            raise ViewStop(f"region {r!r}: reference {ref} is not one of the header's {len(names)}")
        if beg < 0:
            raise ViewStop(f"region {r!r}: BEG is below 1")
        if end < beg:
            raise ViewStop(f"region {r!r}: END is below BEG")
        out.append((ref, beg, min(end, MAX_END)))
    return out


def merge_regions(regions):
    """[(ref_id, beg, end)] -> the same bases as disjoint intervals: sorted, those of one reference that overlap or touch merged, empty
    ones dropped"""
    out = []
    for ref, beg, end in sorted(r for r in regions if r[2] > r[1]):
        if out and out[-1][0] == ref and beg <= out[-1][2]:
            out[-1][2] = max(out[-1][2], end)
        else:
            out.append([ref, beg, end])
    return [tuple(r) for r in out]


# ---- the index ----------------------------------------------------------------------------------------------------------------------------
def read_bai(data):
    """the bytes of a .bai (SAM specification 5.2) -> ([per reference dict(bins={bin: [(beg, end)]}, meta=((beg, end), (mapped, unmapped))
    or None, lin=[..], order=[bin, ..])], n_no_coor or None where the file ends without it).  Any writer's file: bins in any order, the
    pseudo-bin 37450 anywhere or absent."""
    data = bytes(data)
    if data[:4] != b"BAI\x01" or len(data) < 8:
        raise ViewStop("the index does not begin with BAI\\1")
    try:
        n_ref, at = struct.unpack_from("<i", data, 4)[0], 8
        refs = []
        for _ in range(n_ref):
            n_bin = struct.unpack_from("<i", data, at)[0]
            at += 4
            bins, meta, order = {}, None, []
            for _b in range(n_bin):
                bin_id, n_chunk = struct.unpack_from("<Ii", data, at)
                at += 8
                if n_chunk < 0 or at + 16 * n_chunk > len(data):
                    raise struct.error("chunks")
                flat = struct.unpack_from(f"<{2 * n_chunk}Q", data, at)
                chunks = list(zip(flat[0::2], flat[1::2]))
                at += 16 * n_chunk
                order.append(bin_id)
                if bin_id == META_BIN and n_chunk == 2:
                    meta = (chunks[0], chunks[1])
                else:
                    bins.setdefault(bin_id, []).extend(chunks)
            n_intv = struct.unpack_from("<i", data, at)[0]
            if n_intv < 0:
                raise struct.error("windows")
            lin = list(struct.unpack_from(f"<{n_intv}Q", data, at + 4))
            at += 4 + 8 * n_intv
            refs.append(dict(bins=bins, meta=meta, lin=lin, order=order))
        no_coor = None
        if at + 8 <= len(data):
            no_coor = struct.unpack_from("<Q", data, at)[0]
            at += 8
    except struct.error:
        raise ViewStop("the index ends inside an entry")
    if at != len(data):
        raise ViewStop("the index has bytes behind its last entry")
    return refs, no_coor


def _bins_of(beg, end):
    """reg2bins(beg, end) of the specification: the bins a record that overlaps [beg, end) may lie in"""
    last = end - 1
    for first, shift in LEVELS:
        yield from range(first + (beg >> shift), first + (last >> shift) + 1)


def _bin_span(b):
    for first, shift in reversed(LEVELS):
        if b >= first:
            return (b - first) << shift, (b - first + 1) << shift
    return 0, 0


def query_ranges(bai, regions):
    """bai: what read_bai gives (or its first part); regions: merged (ref_id, beg, end) -> the ranges of virtual offsets to read:
    per region the chunks of reg2bins(beg, end), never the pseudo-bin's, without those that end at or before the linear index's value for
    window beg >> 14 (the last window's where beg >> 14 lies behind the windows); their union over all regions sorted, chunks that
    overlap or touch merged.  Disjoint and ascending: each is read once."""
    refs = bai[0] if isinstance(bai, tuple) else bai
    got = []
    for ref, beg, end in regions:
        r = refs[ref]
        end = min(end, MAX_END)
        if end <= beg:
            continue
        w = beg >> 14
        low = r["lin"][w] if w < len(r["lin"]) else (r["lin"][-1] if r["lin"] else 0)
        n_bins = sum(((end - 1) >> shift) - (beg >> shift) + 1 for _first, shift in LEVELS)
        if n_bins <= len(r["bins"]):
            mine = (r["bins"].get(b, ()) for b in _bins_of(beg, end) if b != META_BIN)
        else:                                          # a wide region: the bins the reference has, tested one by one
            mine = (ch for b, ch in r["bins"].items() if b < META_BIN and _bin_span(b)[0] < end and _bin_span(b)[1] > beg)
        for chunks in mine:
            got += [c for c in chunks if c[1] > low and c[1] > c[0]]
    out = []
    for cb, ce in sorted(got):
        if out and cb <= out[-1][1]:
            out[-1][1] = max(out[-1][1], ce)
        else:
            out.append([cb, ce])
    return [tuple(c) for c in out]


def index_path_of(in_bam, index_path=None):
    """the index of in_bam: index_path, else <in>.bai, else <in without .bam>.bai"""
    if index_path is not None:
        if not os.path.isfile(index_path):
            raise ViewStop(f"BamView: a region needs an index: {index_path} does not exist (bamindex.py writes one)")
        return index_path
    a = f"{in_bam}.bai"
    b = (in_bam[:-4] if in_bam.endswith(".bam") else in_bam) + ".bai"
    for p in (a, b):
        if os.path.isfile(p):
            return p
    raise ViewStop(f"BamView: a region needs an index: neither {a} nor {b} exists (bamindex.py writes one)")


# ---- the header ---------------------------------------------------------------------------------------------------------------------------
def read_header(in_bam, n_threads=1):
    """-> (the header's bytes: magic, l_text, text, reference dictionary; its text; [(name, length)]), from as many BGZF blocks of the
    file's front as it takes.  No Context and no GPU."""
    want = 1 << 16
    size = os.path.getsize(in_bam)
    with open(in_bam, "rb") as f:
        while True:
            comp = np.frombuffer(f.read(want), dtype=np.uint8)
            f.seek(0)
            if comp.size < 2 or comp[0] != 0x1F or comp[1] != 0x8B:
                raise _lib.SmiError(f"{in_bam}: not a BGZF file")
            buf, _used = _lib.bgzf_inflate(comp, n_threads=n_threads)
            try:
                text, refs, start = _lib.bam_header(buf)
                return buf[:start].tobytes(), text, refs
            except _lib.SmiError:
                if want >= size:
                    raise
            want *= 4


def header_text(in_bam):
    """the header text of a BAM, as `samtools view -H` prints it"""
    hdr = read_header(in_bam)[0]
    return hdr[8:8 + struct.unpack_from("<I", hdr, 4)[0]].decode("latin-1").rstrip("\0")


def _ref_names(refs):
    return [(r[0].decode("latin-1") if isinstance(r[0], (bytes, bytearray)) else str(r[0])).rstrip("\0") for r in refs]


# ---- the program --------------------------------------------------------------------------------------------------------------------------
def view_bam(ctx, in_bam, out_bam, regions=(), require=0, exclude=0, min_mapq=0, index=False, index_path=None, segment_bytes=256 << 20, n_threads=4):
    """-> dict of counts (records, kept, bytes, bytes_kept, regions, segments), device ms per stage, seconds, bytes written, wall time,
    and of what was read: ranges, blocks_read, compressed_bytes_read.  regions: texts (parse_region) or (name or ref_id, beg0, end0)
    tuples, half-open; none: the whole file is streamed and the filters alone decide.  require / exclude / min_mapq: samtools' -f, -F, -q.
    index: also leave <out_bam>.bai, built from the records and the BGZF blocks as they are written (bamindex.WriterIndex); the info then
    has `index` (None where no index can be built over the output: the BAM is kept and `index_error` says why).  index_path: the input's
    index, where it is neither <in_bam>.bai nor <in_bam without .bam>.bai.  out_bam None: nothing is written (the counts alone)."""
    t_all = time.perf_counter()
    tmp = None if out_bam is None else f"{out_bam}.tmp{os.getpid()}"
    secs = dict(bam_read_inflate=0.0, index=0.0, device=0.0, write=0.0)
    stage_ms = dict.fromkeys(_lib.BAMVIEW_STAGES, 0.0)
    read = dict(ranges=0, blocks_read=0, compressed_bytes_read=0)
    regions = list(regions)
    h = wix = f = None
    written = 0

    def timed(call, *args, **kw):
        t0 = time.perf_counter()
        out = call(*args, **kw)
        secs["device"] += time.perf_counter() - t0
        return out

    def on_blocks(coffset, _isize, end_coffset, _stream_off):
        read["blocks_read"] += int(len(coffset))
        read["compressed_bytes_read"] = int(end_coffset)

    def emit(header=None, bam=None, recs=None):
        """the header's blocks, or the blocks of a segment's kept records, to the file"""
        nonlocal written
        if header is not None:
            if f is None:
                return
            data = np.frombuffer(header, dtype=np.uint8)
            z = timed(ctx.bgzf_deflate_device, data)[:-len(BGZF_EOF)]
        else:
            timed(h.add_segment, bam, recs)
            z, data = timed(h.convert, inflated=wix is not None)
            for k, v in h.stage_ms().items():
                stage_ms[k] += v
            if f is None:
                return
        t0 = time.perf_counter()
        f.write(memoryview(z))
        secs["write"] += time.perf_counter() - t0
        if wix is not None:
            wix.emitted(header if header is not None else data, z, written, records=header is None)
        written += len(z)

    try:
        if regions:                                   # everything that can stop the run is looked at before anything is written
            header, _text, refs = read_header(in_bam, n_threads)
            merged = merge_regions(resolve_regions(regions, _ref_names(refs)))
            path = index_path_of(in_bam, index_path)
            with open(path, "rb") as g:
                try:
                    bai = read_bai(g.read())
                except ViewStop as e:
                    raise ViewStop(f"BamView: {path}: {e}")
            if len(bai[0]) != len(refs):
                raise ViewStop(f"BamView: {path} has {len(bai[0])} references, the header of {in_bam} has {len(refs)}: the index does not belong to the BAM")
            spans = query_ranges(bai, merged)
            read["ranges"] = len(spans)
        if tmp is not None:
            f = open(tmp, "wb")
            if index:
                from .bamindex import WriterIndex
                wix = WriterIndex(ctx)
        if regions:
            emit(header=header)
            if merged:
                h = _lib.BamView(ctx, len(refs), merged, require, exclude, min_mapq)
                try:
                    for bam, recs in bamsegments.ranges(in_bam, spans, segment_bytes, n_threads, secs, stats=read):
                        emit(bam=bam, recs=recs)
                except bamsegments.RangeError as e:
                    raise ViewStop(f"BamView: {path} does not belong to {in_bam}: {e}")
        else:
            for bam, recs, hdr in bamsegments.segments(in_bam, segment_bytes, n_threads, secs, blocks=on_blocks):
                if hdr is not None:
                    _text, refs, _start = _lib.bam_header(np.frombuffer(hdr, dtype=np.uint8))
                    h = _lib.BamView(ctx, len(refs), (), require, exclude, min_mapq)
                    emit(header=hdr)
                if recs.size:
                    emit(bam=bam, recs=recs)
        counts = h.counts() if h is not None else dict.fromkeys(_lib.BAMVIEW_COUNTS, 0)
        info = dict(counts, stage_ms=stage_ms, seconds=secs, bytes_written=0, **read)
        if f is not None:
            f.write(BGZF_EOF)
            written += len(BGZF_EOF)
            f.close()
            f = None
            os.replace(tmp, out_bam)
            info["bytes_written"] = written
            if wix is not None:
                info["index"], info["index_error"] = wix.finish(f"{out_bam}.bai", written - len(BGZF_EOF))
    finally:
        if f is not None:
            f.close()
        if wix is not None:
            wix.close()
        if h is not None:
            h.close()
        if tmp is not None and os.path.exists(tmp):
            os.remove(tmp)
    info["wall_s"] = time.perf_counter() - t_all
    return info


USAGE = "usage: bamview.py [-b] [-S] [-h] [-@ N] [-f INT] [-F INT] [-q INT] [--write-index] -o out.bam in.bam [region ...] | -H in.bam | -c in.bam [region ...]"
NO_EFFECT = {"S": "the input's format is found from its bytes", "h": "the header is always written"}
REFUSED = {"L": "a filter on a BED file", "r": "a filter on read groups", "R": "a filter on read groups", "s": "subsampling", "d": "a filter on a tag",
           "D": "a filter on a tag", "1": "the fast compression level", "u": "uncompressed output", "U": "a file of the records left out",
           "M": "the multi-region iterator", "X": "an index beside the regions"}
WITH_VALUE = "fFqo@O"
BAM_MAGIC = b"\x1f\x8b"


def main(argv=None):
    """-> exit code: 0, or 1 with the message on stderr (argument errors and the stops, named)"""
    from . import cli
    argv = list(sys.argv[1:] if argv is None else argv)
    try:
        if not argv or argv[0] in ("--help", "help"):
            print(__doc__)
            return 0
        got = {}
        binary = only_header = count = write_index = False
        paths = []
        k = 0
        while k < len(argv):
            a = argv[k]
            k += 1
            if a in ("--threads", "--output-fmt", "--output"):
                if k >= len(argv):
                    raise cli.CliError(f"{a} needs a value; {USAGE}")
                got[{"--threads": "@", "--output-fmt": "O", "--output": "o"}[a]] = argv[k]
                k += 1
            elif a == "--write-index":
                write_index = True
            elif a == "-" or not a.startswith("-"):
                paths.append(a)
            elif a.startswith("--"):
                raise cli.CliError(f"unknown option {a!r}; {USAGE}")
            else:                                          # a cluster of flags; one that takes a value ends it
                j = 1
                while j < len(a):
                    c = a[j]
                    j += 1
                    if c in WITH_VALUE:
                        if j < len(a):
                            got[c] = a[j:]
                        elif k < len(argv):
                            got[c] = argv[k]
                            k += 1
                        else:
                            raise cli.CliError(f"-{c} needs a value; {USAGE}")
                        break
                    if c == "b":
                        binary = True
                    elif c == "H":
                        only_header = True
                    elif c == "c":
                        count = True
                    elif c in REFUSED:
                        raise cli.CliError(f"-{c}: {REFUSED[c]} is not built: bamview.py filters by region, flag bits and MAPQ")
                    elif c not in NO_EFFECT:
                        raise cli.CliError(f"unknown option -{c} in {a!r}; {USAGE}")

        def number(c, what, top):
            if c not in got:
                return 0
            t = got[c]
            try:
                v = int(t, 16) if t.lower().startswith("0x") and c in "fF" else int(t, 10)
            except ValueError:
                raise cli.CliError(f"-{c} {t!r}: not a number")
            if not 0 <= v <= top:
                raise cli.CliError(f"-{c} {v}: not {what}")
            return v

        fmt, out_bam = got.get("O"), got.get("o")
        if fmt is not None and fmt.lower() != "bam":
            raise cli.CliError(f"-O {fmt}: this build writes BAM alone")
        require, exclude, min_mapq = number("f", "flag bits", 0xFFFF), number("F", "flag bits", 0xFFFF), number("q", "a MAPQ", 255)
        threads = number("@", "a thread count", 1 << 16) if "@" in got else None
        if not paths:
            raise cli.CliError(USAGE)
        in_bam, regions = paths[0], paths[1:]
        if not only_header and not count:
            if not binary and fmt is None:
                raise cli.CliError(f"-b is missing: this build writes BAM alone; {USAGE}")
            if out_bam is None:
                raise cli.CliError(f"-o is missing: this build writes a file, not the standard output; {USAGE}")
        if in_bam == "-":
            raise cli.CliError("-: the input is a file in this build, not the standard input")
        if not os.path.isfile(in_bam):
            raise cli.CliError(f"{in_bam}: no such file")
        with open(in_bam, "rb") as f:
            if f.read(2) != BAM_MAGIC:
                raise cli.CliError(f"{in_bam}: not a BAM: this build reads BAM here (samview.py converts SAM text)")
        if out_bam is not None and (not os.path.isdir(os.path.dirname(os.path.abspath(out_bam))) or os.path.isdir(out_bam)):
            raise cli.CliError(f"{out_bam}: no such directory, or a directory")
        if only_header:
            text = header_text(in_bam)
            if out_bam is None:
                sys.stdout.write(text)
                sys.stdout.flush()
            else:
                with open(out_bam, "w", encoding="latin-1", newline="") as f:
                    f.write(text)
            return 0
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise cli.CliError("bamview.py runs in one process on one GPU in this build: start it without torchrun")
        n_threads = max(1, min(threads, 16)) if threads else cli._ncpu({})       # samtools' -@ counts additional threads; 0 = none
        try:
            info = view_bam(cli._context(), in_bam, None if count else out_bam, regions, require, exclude, min_mapq, index=write_index and not count,
                            n_threads=n_threads)
        except (_lib.BamViewError, ViewStop) as e:
            raise cli.CliError(f"{in_bam}: {e}" + ("" if count else f"; {out_bam} was not written"))
        if count:
            if out_bam is None:
                print(info["kept"])
            else:
                with open(out_bam, "w") as f:
                    f.write(f"{info['kept']}\n")
            return 0
        print(f"DONE -- {info['kept']} of {info['records']} records kept in {info['segments']} segments, {info['ranges']} ranges and {info['blocks_read']} "
              f"blocks read, {info['bytes_written']} bytes written", file=sys.stderr)
        if info.get("index_error"):
            print(f"WARNING: {info['index_error']}", file=sys.stderr)
        return 0
    except cli.CliError as e:
        print(f"ERROR: {e}", file=sys.stderr)
        return 1
    except (_lib.SmiError, OSError, ValueError) as e:
        print(f"ERROR: {type(e).__name__}: {e}", file=sys.stderr)
        return 1
