"""Independent Python model of BamIndex: the .bai of a coordinate-sorted BAM in this build's canonical form, restated
from the definition over a BAM file's bytes, and the specification's reader of the format (SAM specification 5.2 / 5.3).  Test
infrastructure only."""
import bisect
import struct
import zlib

import numpy as np

import bammodel

META_BIN = 37450
MAX_END = 1 << 29
REF_OPS = "MDN=X"


class BaiStop(Exception):
    """a record no index is built over: .record (0-based), .read, .kind (order, negative, far, ref, past)"""

    def __init__(self, record, read, kind):
        super().__init__(f"record {record} ({read}): {kind}")
        self.record, self.read, self.kind = record, read, kind


def bgzf_walk(raw):
    """-> [(coffset, block size, inflated bytes)] of a BGZF file, by its own walk over the gzip members"""
    out, off = [], 0
    while off < len(raw):
        assert raw[off:off + 4] == b"\x1f\x8b\x08\x04", off
        xlen = struct.unpack_from("<H", raw, off + 10)[0]
        x, bsize = off + 12, None
        while x < off + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", raw, x)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", raw, x + 4)[0] + 1
            x += 4 + slen
        payload = zlib.decompress(raw[off + 12 + xlen:off + bsize - 8], -15)
        assert len(payload) == struct.unpack_from("<I", raw, off + bsize - 4)[0]
        out.append((off, bsize, payload))
        off += bsize
    return out


def offsets_of(raw):
    """-> (inflated stream, f) with f(p) = the virtual offset of inflated position p (p = the stream's length: behind the last byte)"""
    blocks = [b for b in bgzf_walk(raw) if b[2]]          # empty blocks hold no byte
    starts, at = [], 0
    for _c, _s, payload in blocks:
        starts.append(at)
        at += len(payload)
    total = at

    def voff(p):
        assert 0 <= p <= total
        if p == total:
            return (blocks[-1][0] + blocks[-1][1]) << 16 if blocks else 0
        k = bisect.bisect_right(starts, p) - 1
        return blocks[k][0] << 16 | (p - starts[k])

    return b"".join(b[2] for b in blocks), voff


def extent(rec):
    """[beg, end) of a parse_bam record: the stored CIGAR as it stands; one base for an empty one and for flag 0x4"""
    n = sum(ln for op, ln in rec["cigar"] if op in REF_OPS)
    if n == 0 or rec["flag"] & 4:
        n = 1
    return rec["pos0"], rec["pos0"] + n


def windows_of(ref_len):
    """the 16 kb windows the header's length gives a reference"""
    return min(1 << 15, ((max(ref_len, 1) - 1) >> 14) + 1)


def records_of(raw):
    """-> (refs, [(ref_id, beg, end, flag, virtual offset, virtual offset behind, name)]) in file order"""
    data, voff = offsets_of(raw)
    _text, refs, recs = bammodel.parse_bam(data)
    out = []
    for r in recs:
        beg, end = extent(r)
        out.append((r["ref_id"], beg, end, r["flag"], voff(r["off"]), voff(r["off"] + r["length"]), r["name"]))
    return refs, out


def check_order(refs, recs):
    """raises BaiStop at the first record the definition stops at"""
    prev = None
    for i, (ref, beg, end, _flag, _vb, _ve, name) in enumerate(recs):
        if ref >= 0:
            if beg < 0:
                raise BaiStop(i, name, "negative")
            if end > MAX_END:
                raise BaiStop(i, name, "far")
            if ref >= len(refs):
                raise BaiStop(i, name, "ref")
            if (end - 1) >> 14 >= windows_of(refs[ref][1]):
                raise BaiStop(i, name, "past")
        key = (1, 0, 0) if ref < 0 else (0, ref, beg)
        if prev is not None and key < prev:
            raise BaiStop(i, name, "order")
        prev = key


def bai_model(raw):
    """the .bai of the BAM file `raw` (bytes); BaiStop where the definition stops"""
    refs, recs = records_of(raw)
    check_order(refs, recs)
    n_ref = len(refs)
    chunks = [dict() for _ in range(n_ref)]           # bin -> [[beg, end]] in file order
    lin = [dict() for _ in range(n_ref)]
    meta = [None] * n_ref                             # [min offset, max end offset, mapped, flag 0x4, largest end]
    no_coor, last = 0, None
    for ref, beg, end, flag, vb, ve, _name in recs:
        if ref < 0:
            no_coor += 1
            last = None
            continue
        b = bammodel.reg2bin(beg, end)
        if last == (ref, b):
            chunks[ref][b][-1][1] = ve                # the run goes on
        else:
            chunks[ref].setdefault(b, []).append([vb, ve])
        last = (ref, b)
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            lin[ref][w] = min(lin[ref].get(w, vb), vb)
        m = meta[ref] or [vb, ve, 0, 0, end]
        meta[ref] = [min(m[0], vb), max(m[1], ve), m[2] + (0 if flag & 4 else 1), m[3] + (1 if flag & 4 else 0), max(m[4], end)]
    out = [b"BAI\x01", struct.pack("<i", n_ref)]
    for ref in range(n_ref):
        m = meta[ref]
        out.append(struct.pack("<i", len(chunks[ref]) + (1 if m else 0)))
        for b in sorted(chunks[ref]):
            out.append(struct.pack("<Ii", b, len(chunks[ref][b])))
            out += [struct.pack("<QQ", cb, ce) for cb, ce in chunks[ref][b]]
        n_intv = 0
        if m:
            out.append(struct.pack("<IiQQQQ", META_BIN, 2, m[0], m[1], m[2], m[3]))
            n_intv = ((m[4] - 1) >> 14) + 1
        out.append(struct.pack("<i", n_intv))
        v = 0
        for w in range(n_intv):
            v = lin[ref].get(w, v)
            out.append(struct.pack("<Q", v))
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


def parse_bai(b):
    """-> ([{bins: {bin: [(beg, end)]}, meta: ((beg, end), (mapped, flag4)) or None, lin: [..]}], n_no_coor or None); every byte is read"""
    assert b[:4] == b"BAI\x01"
    n_ref, at = struct.unpack_from("<i", b, 4)[0], 8
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", b, at)[0]
        at += 4
        bins, meta, order = {}, None, []
        for _b in range(n_bin):
            bin_id, n_chunk = struct.unpack_from("<Ii", b, at)
            at += 8
            ch = [struct.unpack_from("<QQ", b, at + 16 * c) for c in range(n_chunk)]
            at += 16 * n_chunk
            order.append(bin_id)
            if bin_id == META_BIN:
                assert n_chunk == 2
                meta = (ch[0], ch[1])
            else:
                assert bin_id not in bins
                bins[bin_id] = ch
        n_intv = struct.unpack_from("<i", b, at)[0]
        lin = list(struct.unpack_from("<%dQ" % n_intv, b, at + 4))
        at += 4 + 8 * n_intv
        refs.append(dict(bins=bins, meta=meta, lin=lin, order=order))
    no_coor = None
    if at < len(b):
        no_coor = struct.unpack_from("<Q", b, at)[0]
        at += 8
    assert at == len(b)
    return refs, no_coor


def reg2bins(beg, end):
    """the bins that may hold a record overlapping [beg, end) (SAM specification 5.3)"""
    end -= 1
    out = [0]
    for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(base + (beg >> shift), base + (end >> shift) + 1)
    return out


def bai_query(bai, ref, beg, end):
    """the specification's reader: the chunks of reg2bins(beg, end) that end behind the linear index's lower bound, in file order.
    bai: the file's bytes, or what parse_bai made of them"""
    refs = parse_bai(bai)[0] if isinstance(bai, (bytes, bytearray)) else bai
    r = refs[ref]
    w = beg >> 14
    low = r["lin"][w] if w < len(r["lin"]) else (r["lin"][-1] if r["lin"] else 0)
    got = [c for b in reg2bins(beg, end) for c in r["bins"].get(b, ()) if c[1] > low]
    return sorted(got)


def uncovered(raw, bai, regions=()):
    """the cover property: for every record's own extent and for every (ref, beg, end) of `regions`, each record that overlaps the region
    must lie inside the chunks bai_query returns -> the list of (region, record number) that do not"""
    _refs, recs = records_of(raw)
    parsed = parse_bai(bai)[0]
    per_ref = {}
    for i, r in enumerate(recs):
        if r[0] >= 0:
            per_ref.setdefault(r[0], []).append((i, r[1], r[2], r[4], r[5]))
    per_ref = {k: np.array(v, dtype=np.uint64).T for k, v in per_ref.items()}
    bad = []
    todo = dict.fromkeys([(r[0], r[1], r[2]) for r in recs if r[0] >= 0] + list(regions))
    for ref, beg, end in todo:
        chunks = bai_query(parsed, ref, beg, end)
        if ref not in per_ref:
            continue
        idx, rb, re_, vb, ve = per_ref[ref]
        hit = (rb < np.uint64(end)) & (re_ > np.uint64(beg))
        ok = np.zeros(hit.shape, dtype=bool)
        for cb, ce in chunks:
            ok |= (vb >= np.uint64(cb)) & (ve <= np.uint64(ce))
        bad += [((ref, beg, end), int(i)) for i in idx[hit & ~ok]]
    return bad
