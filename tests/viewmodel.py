"""Independent Python model of BamView: a full scan of the inflated stream with the overlap and filter rules, which
uses no index; the region grammar; and the range rule, the BGZF blocks under the merged chunks of baimodel.bai_query, counted.  A product
that reads through an index must equal the scan.  Test infrastructure only."""
import re

import baimodel
import bammodel

MAX_END = 1 << 29
NUMBER = re.compile(r"[0-9,]*[0-9][0-9,]*")          # decimal digits, commas anywhere among them


class RegionStop(Exception):
    """.kind: name, beg, end, number"""

    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


def parse_region(text, names):
    """-> (ref_id, beg, end) half-open and 0-based; RegionStop where the definition stops"""
    if text in names:
        return names.index(text), 0, MAX_END
    if ":" not in text:
        raise RegionStop("name")
    name, span = text[:text.rindex(":")], text[text.rindex(":") + 1:]
    if name not in names:
        raise RegionStop("name")
    parts = span.split("-", 1)
    for p in parts:
        if not NUMBER.fullmatch(p):
            raise RegionStop("number")
    nums = [int(p.replace(",", "")) for p in parts]
    if nums[0] < 1:
        raise RegionStop("beg")
    if len(nums) == 2 and nums[1] < nums[0]:
        raise RegionStop("end")
    return names.index(name), nums[0] - 1, min(nums[1], MAX_END) if len(nums) == 2 else MAX_END


def merged(regions):
    """disjoint intervals: the regions of one reference that overlap or touch become one; empty ones cover nothing"""
    out = []
    for ref, b, e in sorted(set(r for r in regions if r[2] > r[1])):
        if out and out[-1][0] == ref and b <= out[-1][2]:
            out[-1] = (ref, out[-1][1], max(out[-1][2], e))
        else:
            out.append((ref, b, e))
    return out


def overlaps(rec, regions):
    if rec["ref_id"] < 0:
        return False
    beg, end = baimodel.extent(rec)
    return any(rec["ref_id"] == ref and beg < e and end > b for ref, b, e in regions)


def passes(rec, require=0, exclude=0, min_mapq=0):
    return rec["flag"] & require == require and not rec["flag"] & exclude and rec["mapq"] >= min_mapq


def scan(raw, regions=None, require=0, exclude=0, min_mapq=0):
    """the full scan -> (the header's bytes, [kept record bytes], [kept record numbers], all records); regions None: the filters alone"""
    data = bammodel.bgzf_decompress(raw)
    _text, _refs, recs = bammodel.parse_bam(data)
    start = recs[0]["off"] if recs else len(data)
    kept = [k for k, r in enumerate(recs) if passes(r, require, exclude, min_mapq) and (regions is None or overlaps(r, regions))]
    return data[:start], [data[recs[k]["off"]:recs[k]["off"] + recs[k]["length"]] for k in kept], kept, recs


def view(raw, regions=None, **filters):
    """the inflated bytes of the product: the input's header, the kept records, nothing else"""
    header, kept, _idx, _recs = scan(raw, regions, **filters)
    return header + b"".join(kept)


def ranges(bai, regions):
    """the ranges of virtual offsets a reader of the index reads for the merged regions: the chunks of baimodel.bai_query over all of
    them (empty chunks hold nothing), sorted, those that overlap or touch merged"""
    parsed = baimodel.parse_bai(bai)[0] if isinstance(bai, (bytes, bytearray)) else bai
    chunks = sorted(set(c for ref, b, e in merged(regions) for c in baimodel.bai_query(parsed, ref, b, e) if c[1] > c[0]))
    out = []
    for cb, ce in chunks:
        if out and cb <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], ce))
        else:
            out.append((cb, ce))
    return out


def blocks_under(raw, rngs):
    """-> (blocks, compressed bytes) read for the ranges: of each range the block of its begin up to the block that holds the byte in front
    of its end; a block several ranges share is read once"""
    walk = baimodel.bgzf_walk(raw)
    mine = {}
    for vb, ve in rngs:
        cb, ce, ue = vb >> 16, ve >> 16, ve & 0xFFFF
        for coff, bsize, _payload in walk:
            if cb <= coff and (coff < ce or (ue and coff == ce)):
                mine[coff] = bsize
    return len(mine), sum(mine.values())


def seen(raw, rngs):
    """the numbers of the records that lie inside the ranges: what the device is handed"""
    _refs, recs = baimodel.records_of(raw)
    return [k for k, r in enumerate(recs) if any(vb <= r[4] and r[5] <= ve for vb, ve in rngs)]


def counts(raw, bai=None, regions=None, **filters):
    """records, kept, bytes, bytes_kept, regions as the product counts them"""
    _header, kept, idx, recs = scan(raw, regions, **filters)
    if regions is None:
        mine = list(range(len(recs)))
    else:
        mine = seen(raw, ranges(bai, regions))
        assert set(idx) <= set(mine), "the cover property fails"
    return dict(records=len(mine), kept=len(kept), bytes=sum(recs[k]["length"] for k in mine), bytes_kept=sum(len(b) for b in kept),
                regions=len(merged(regions)) if regions is not None else 0)
