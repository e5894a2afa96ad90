"""Plain-Python model of `tagbamwithread` (TagWithReadSequenceMain.doJob L85-116 over ReadNameChrHashMap / SplitFastqByChromosome): the
records of an inflated BAM, each dropped, reported or tagged with its read's bases / qualities as htsjdk writes it.  The attribute rules are
assignumis.split_aux / apply_tag_sets, which tests/golden/ref_exec_auxorder.json pins.  Test infrastructure only."""
import importlib
import struct

import __graft_entry__ as graft

MISS = "ERROR: Did not find read for  SAM record, name: {} Check whether fastq and BAM file correspond !"


def fastq_map(text):
    """FASTQ text -> {key: (bases, qualities)}: key = the header line without '@' cut at its first SPACE (a tab stays); a name that occurs
    twice keeps its last record (HashMap.put)"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]
    assert len(lines) % 4 == 0, "truncated FASTQ"
    out = {}
    for i in range(0, len(lines), 4):
        assert lines[i][:1] == b"@" and lines[i + 2][:1] == b"+" and len(lines[i + 1]) == len(lines[i + 3]), "malformed FASTQ"
        out[lines[i][1:].split(b" ")[0]] = (lines[i + 1], lines[i + 3])
    return out


def records_start(bam):
    l_text = struct.unpack_from("<I", bam, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<I", bam, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<I", bam, p)[0]
    return p


def tag_bam(fastq_text, bam, read_tag, qv_tag=None):
    """-> (inflated output BAM, [miss lines], dict of counts)"""
    graft.load_package()
    au = importlib.import_module(graft.PKG_NAME + ".assignumis")
    reads = fastq_map(fastq_text)
    p = records_start(bam)
    out, miss = [bam[:p]], []
    counts = dict(records=0, written=0, unmapped=0, missing=0)
    while p < len(bam):
        bs = struct.unpack_from("<I", bam, p)[0]
        body = bam[p + 4:p + 4 + bs]
        p += 4 + bs
        counts["records"] += 1
        ref_id = struct.unpack_from("<i", body, 0)[0]
        l_nm, n_cig, l_seq = body[8], struct.unpack_from("<H", body, 12)[0], struct.unpack_from("<i", body, 16)[0]
        name = body[32:32 + l_nm - 1] if l_nm else b""
        if ref_id == -1:
            counts["unmapped"] += 1
            continue
        if name not in reads:
            counts["missing"] += 1
            miss.append(MISS.format(name.decode("latin-1")))
            continue
        seq, qual = reads[name]
        a = 32 + l_nm + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        calls = [(read_tag, seq.decode())] + ([(qv_tag, qual.decode())] if qv_tag else [])
        fields = au.apply_tag_sets(au.split_aux(body[a:]), calls)
        new = body[:a] + b"".join(raw for _, raw in fields)
        out.append(struct.pack("<I", len(new)) + new)
        counts["written"] += 1
    return b"".join(out), miss, counts


# ---- attribute builders for fixtures ------------------------------------------------------------------------------------------------------
def aux_z(tag, s):
    return tag.encode() + b"Z" + s.encode() + b"\0"


def aux_int(tag, code, v):
    fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[code]
    return tag.encode() + code.encode() + struct.pack(fmt, v)


def aux_h(tag, hexdigits):
    return tag.encode() + b"H" + hexdigits.encode() + b"\0"


def aux_b(tag, code, values):
    fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[code]
    return tag.encode() + b"B" + code.encode() + struct.pack("<I", len(values)) + struct.pack("<%d%s" % (len(values), fmt), *values)


def aux_a(tag, ch):
    return tag.encode() + b"A" + ch.encode()


def aux_f(tag, v):
    return tag.encode() + b"f" + struct.pack("<f", v)


def fastq_text(rows):
    """rows: [(header line without '@', bases, qualities)]"""
    return b"".join(b"@" + h.encode() + b"\n" + s.encode() + b"\n+\n" + q.encode() + b"\n" for h, s, q in rows)
