"""The definition of BamSort's order in plain Python, on bammodel's parser: the key, Python's stable sorted(), the
header rule, the stop and the output windows.  Test infrastructure only; it shares nothing with the product."""
import struct

import bammodel


class SortStop(Exception):
    """a record the sort stops at (a ref_id that is none of the header's): .record (0-based), .read"""

    def __init__(self, record, read):
        super().__init__(f"read {read} (record {record})")
        self.record, self.read = record, read


def key(rec, n_ref):
    """(reference rank, pos + 1 as an unsigned 32-bit number, reverse-strand bit) of a parse_bam record"""
    ref = rec["ref_id"]
    return (ref if 0 <= ref < n_ref else n_ref, (rec["pos0"] + 1) & 0xFFFFFFFF, (rec["flag"] >> 4) & 1)


def header_text(text):
    """the header text with SO:coordinate"""
    line, nl, after = text.partition("\n")
    fields = line.split("\t")
    if fields[0] != "@HD":
        return "@HD\tVN:1.6\tSO:coordinate\n" + text
    for k in range(1, len(fields)):
        if fields[k].startswith("SO:"):
            fields[k] = "SO:coordinate"
            break
    else:
        fields.append("SO:coordinate")
    return "\t".join(fields) + nl + after


def split(data):
    """the inflated BAM -> (text, bytes of the reference dictionary from n_ref on, refs, records of parse_bam)"""
    text, refs, recs = bammodel.parse_bam(data)
    l_text = struct.unpack_from("<I", data, 4)[0]
    p = 8 + l_text + 4
    for _ in refs:
        p += 8 + struct.unpack_from("<I", data, p)[0]
    return text, data[8 + l_text:p], refs, recs


def sorted_records(data):
    """-> (header bytes, [record bytes] in sorted order); SortStop at the first ref_id >= n_ref"""
    text, dictionary, refs, recs = split(data)
    for i, r in enumerate(recs):
        if r["ref_id"] >= len(refs):
            raise SortStop(i, r["name"])
    t = header_text(text).encode()
    order = sorted(recs, key=lambda r: key(r, len(refs)))
    return b"BAM\1" + struct.pack("<I", len(t)) + t + dictionary, [data[r["off"]:r["off"] + r["length"]] for r in order]


def sorted_stream(raw):
    """the BAM file `raw` (BGZF bytes) -> the inflated bytes of the sorted file"""
    header, records = sorted_records(bammodel.bgzf_decompress(raw))
    return header + b"".join(records)


def windows(lengths, window_bytes):
    """the output windows over records of these lengths in sorted order: as many whole records as window_bytes hold, at least one
    -> [(first rank, rank behind the last, bytes)]"""
    out, b = [], 0
    while b < len(lengths):
        e, size = b + 1, lengths[b]
        while e < len(lengths) and size + lengths[e] <= window_bytes:
            size += lengths[e]
            e += 1
        out.append((b, e, size))
        b = e
    return out
