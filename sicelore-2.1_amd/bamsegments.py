"""The BAM reader of the file programs: a BGZF file in segments of about segment_bytes compressed bytes, inflated one segment ahead by a
reader thread (smi_bgzf_inflate, host threads), the records of each segment indexed (smi_bam_index_records).  A block cut by the end of a
segment is carried to the next one, the header may span segments, and so may a record: its bytes are carried until it is complete."""
import os
import queue
import threading
import time

import numpy as np

from . import lib as _lib

# the empty BGZF block that ends a file
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def segments(in_bam, segment_bytes, n_threads, secs=None, blocks=None):
    """(inflated bytes, records, header bytes or None) per segment: the header's bytes come with the first segment.  secs: a dict whose
    bam_read_inflate (the reader thread's reading and inflating) and index (the record index) grow by the seconds spent.  blocks: a
    function called once per buffer read, before the buffer's segment (if it gives one) is yielded, as blocks(coffset, isize, end_coffset,
    stream_off): the table of the BGZF blocks inflated into it (lib.bgzf_block_table, file offsets), the file offset behind them, and the
    offset in the inflated stream of the first byte of the segment's bytes."""
    inflated = queue.Queue(maxsize=1)
    secs = {} if secs is None else secs

    def reader():
        try:
            with open(in_bam, "rb") as f:
                tail = np.zeros(0, dtype=np.uint8)
                at = 0                                   # file offset of comp[0]
                while True:
                    t1 = time.perf_counter()
                    raw = np.fromfile(f, dtype=np.uint8, count=int(segment_bytes))
                    last = raw.size < int(segment_bytes)
                    comp = np.concatenate([tail, raw]) if tail.size else raw
                    buf, used = _lib.bgzf_inflate(comp, n_threads=n_threads) if comp.size else (np.zeros(0, dtype=np.uint8), 0)
                    table = None
                    if blocks is not None:
                        coff, isize, _used = _lib.bgzf_block_table(comp[:used], base=at)
                        table = (coff, isize, at + used)
                        at += used
                    tail = comp[used:].copy()
                    if last and tail.size:
                        raise _lib.SmiError(f"{in_bam}: truncated BGZF stream")
                    dt = time.perf_counter() - t1
                    del raw, comp               # freed before the consumer is woken: unmapping them beside its page faults stalls the record index
                    inflated.put((buf, last, None, dt, table))
                    if last:
                        return
        except BaseException as e:  # noqa: BLE001 -- handed to the consumer
            inflated.put((None, True, e, 0.0, None))

    threading.Thread(target=reader, daemon=True).start()
    pend = np.zeros(0, dtype=np.uint8)
    header = False
    eof = False
    inflated_before = 0
    while not eof:
        buf, eof, e, dt, table = inflated.get()
        if e is not None:
            raise e
        secs["bam_read_inflate"] = secs.get("bam_read_inflate", 0.0) + dt
        if blocks is not None:
            blocks(*table, inflated_before - pend.size)
        inflated_before += buf.size
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
        hdr = bam[:start].tobytes() if start else None
        t1 = time.perf_counter()
        recs, end = _lib.bam_index_records(bam, start, cap=max(1, (bam.size - start) // 36))
        if eof and end != bam.size:
            raise _lib.SmiError(f"{in_bam}: truncated BAM record")
        secs["index"] = secs.get("index", 0.0) + time.perf_counter() - t1
        if recs.size or hdr is not None:
            yield bam, recs, hdr
        pend = bam[end:].copy()
    if not header:
        raise _lib.SmiError(f"{in_bam}: no BAM header")


class RangeError(_lib.SmiError):
    """the bytes under a range of virtual offsets are no whole records: the index the ranges came from is not this file's"""


def _block_end(fd, coffset, size, what):
    """the file offset behind the BGZF block at coffset, from its header (BSIZE in the BC subfield)"""
    head = os.pread(fd, 12, coffset)
    if len(head) < 12 or head[:4] != b"\x1f\x8b\x08\x04":
        raise RangeError(f"{what}: no BGZF block at file offset {coffset}")
    extra = os.pread(fd, int.from_bytes(head[10:12], "little"), coffset + 12)
    x = 0
    while x + 4 <= len(extra):
        slen = int.from_bytes(extra[x + 2:x + 4], "little")
        if extra[x:x + 2] == b"BC" and slen == 2 and x + 6 <= len(extra):
            end = coffset + int.from_bytes(extra[x + 4:x + 6], "little") + 1
            if end > size:
                raise RangeError(f"{what}: the BGZF block at file offset {coffset} ends behind the file")
            return end
        x += 4 + slen
    raise RangeError(f"{what}: no BGZF block at file offset {coffset}")


def ranges(in_bam, ranges, segment_bytes, n_threads, secs=None, stats=None):
    """(inflated bytes, records) per segment of the records under `ranges`: (begin, end) pairs of virtual offsets (SAM specification 4.1.1),
    ascending and disjoint, each beginning at a record's first byte and ending behind a record's last.  Only the BGZF blocks under the
    ranges are read and inflated: of every range the block of its begin up to the block that holds the byte in front of its end, the
    first from the range's offset inside it on; a block in which one range ends and the next begins is read once.  A segment holds as many whole ranges as fit into segment_bytes of compressed input (at
    least one); a range larger than that is cut at block borders, and the record the cut goes through is carried to the next segment.
    A range whose bytes are no whole records (a block_size below 32, a record that runs past the range's end, a file offset outside the
    file or one that is no block's) raises RangeError, which names the range.  secs: as for segments().  stats: a dict whose blocks_read
    and compressed_bytes_read grow by the blocks inflated and their size in the file."""
    secs = {} if secs is None else secs
    stats = {} if stats is None else stats
    stats.setdefault("blocks_read", 0)
    stats.setdefault("compressed_bytes_read", 0)
    segment_bytes = max(int(segment_bytes), 1)
    size = os.path.getsize(in_bam)
    fd = os.open(in_bam, os.O_RDONLY)
    held = []                                                # the last block inflated: its file offset, its bytes, its size in the file

    def piece(what, at, want, c_end):
        """the whole blocks of file[at .. at + want), at least one -> (inflated bytes, the last block's inflated size, compressed bytes used)"""
        while True:
            comp = np.frombuffer(os.pread(fd, want, at), dtype=np.uint8)
            if comp.size < want:
                raise RangeError(f"{what}: file offset {at + want} is outside the file")
            try:
                _coff, isize, used = _lib.bgzf_block_table(comp, base=at)
                if not used and want < c_end - at:           # a block larger than segment_bytes
                    want = min(c_end - at, want + (1 << 16))
                    continue
                if not used:
                    raise RangeError(f"{what}: no BGZF block at file offset {at}")
                buf, used2 = _lib.bgzf_inflate(comp[:used], n_threads=n_threads)
            except RangeError:
                raise
            except _lib.SmiError as e:
                raise RangeError(f"{what}: {e}")
            if used2 != used:
                raise RangeError(f"{what}: no BGZF block at file offset {at + used2}")
            stats["blocks_read"] += int(isize.size)
            stats["compressed_bytes_read"] += int(used)
            held[:] = [int(_coff[-1]), buf[buf.size - int(isize[-1]):].copy(), at + int(used) - int(_coff[-1])]
            return buf, int(isize[-1]), int(used)

    def index(what, data, whole):
        """the records of data -> (entries, the offset behind the last whole one); the room for the entries is guessed from 64 bytes a
        record and, where that does not hold them, taken from the 36 bytes of the shortest record"""
        t1 = time.perf_counter()
        try:
            recs, end = np.zeros(0, dtype=_lib.BAM_RECORD_DTYPE), 0
            for cap in (data.size // 64 + 16, data.size // 36 + 1):
                if not data.size:
                    break
                recs, end = _lib.bam_index_records(data, 0, cap=cap)
                if recs.size < cap:                              # (the walk ended at the bytes' end, not at the room's)
                    break
        except _lib.SmiError as e:
            raise RangeError(f"{what}: {e}")
        secs["index"] = secs.get("index", 0.0) + time.perf_counter() - t1
        if whole and end != data.size:
            raise RangeError(f"{what}: a record runs past the range's end")
        return recs, end

    def extent(what, vb, ve):
        """-> the file offsets [cb, c_end) of the blocks under the range"""
        cb, ce, ue = vb >> 16, ve >> 16, ve & 0xFFFF
        if cb >= size or ce > size or (ue and ce >= size):
            raise RangeError(f"{what}: file offset {max(cb, ce)} is outside the file")
        if not ue:
            return cb, ce
        return cb, held[0] + held[2] if held and held[0] == ce else _block_end(fd, ce, size, what)

    def one(what, vb, ve, cb, c_end):
        """the inflated bytes of one range in pieces of at most segment_bytes compressed bytes -> (bytes, last piece, whether the piece is
        the block held from the range before) per piece"""
        ub, ue = vb & 0xFFFF, ve & 0xFFFF
        at, first = cb, True
        while at < c_end:
            t1 = time.perf_counter()
            from_held = bool(first and held and held[0] == cb)   # the block the range before ended in: it is not read again
            if from_held:
                buf, last_isize, used = held[1], int(held[1].size), held[2]
            else:
                buf, last_isize, used = piece(what, at, min(c_end - at, segment_bytes), c_end)
            secs["bam_read_inflate"] = secs.get("bam_read_inflate", 0.0) + time.perf_counter() - t1
            at += used
            last = at >= c_end
            lo = ub if first else 0
            hi = buf.size - (last_isize - ue) if last and ue else buf.size
            if (last and ue > last_isize) or lo > hi:
                raise RangeError(f"{what}: an offset behind the end of its block")
            first = False
            yield buf[lo:hi], last, from_held

    def joined(batch):
        """the ranges of a segment one behind the other, the offsets of their records moved along"""
        if len(batch) == 1:
            return batch[0]
        at = 0
        for data, recs in batch:
            for k in ("rec_off", "name_off", "cigar_off", "seq_off", "qual_off", "aux_off"):
                recs[k] += at
            at += data.size
        return np.concatenate([b[0] for b in batch]), np.concatenate([b[1] for b in batch])

    try:
        batch, room = [], segment_bytes                          # whole ranges that share a segment, in file order
        for vb, ve in ranges:
            vb, ve = int(vb), int(ve)
            if ve <= vb:
                continue
            what = f"the range {vb >> 16}:{vb & 0xFFFF} .. {ve >> 16}:{ve & 0xFFFF}"
            cb, c_end = extent(what, vb, ve)
            span = c_end - cb                                    # the compressed bytes of the blocks under the range
            if span > room:                                      # nothing of this range leaves before the ranges in front of it have
                if batch:
                    yield joined(batch)
                batch, room = [], segment_bytes
            if span <= room:                                     # a whole range (the held block and one read at the most): it waits for its neighbours
                parts = [d for d, _last, _held in one(what, vb, ve, cb, c_end)]
                data = np.concatenate(parts) if len(parts) > 1 else parts[0]
                recs = index(what, data, True)[0]
                if recs.size:
                    batch.append((data, recs))
                room -= span
                continue
            pend = np.zeros(0, dtype=np.uint8)                   # a range beyond a segment (the batch is empty): cut at block borders
            for data, last, from_held in one(what, vb, ve, cb, c_end):
                data = np.concatenate([pend, data]) if pend.size else data
                if from_held and not last:                       # (the held block goes with the first read)
                    pend = data
                    continue
                recs, end = index(what, data, last)
                if recs.size:
                    yield data, recs
                pend = data[end:].copy()
        if batch:
            yield joined(batch)
    finally:
        os.close(fd)
