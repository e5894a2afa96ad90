"""The BAM reader of the file programs: a BGZF file in segments of about segment_bytes compressed bytes, inflated one segment ahead by a
reader thread (smi_bgzf_inflate, host threads), the records of each segment indexed (smi_bam_index_records).  A block cut by the end of a
segment is carried to the next one, the header may span segments, and so may a record: its bytes are carried until it is complete."""
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
