"""Plain-Python model of `ExportClippedReads` (ExportClippedReads.java:L50-104) and `AddBamReadTags` (AddBamReadTags.java:L38-72) over an
inflated BAM: the FASTQ / the BAM as the reference writes it, the counters, and the record on which ExportClippedReads' loop dies.  The
loop below restates the Java lines one by one (String.split, the two regex splits of the CIGAR text, the casts); record bytes come from
tests/bammodel.py, the attribute list from tests/moltagmodel.py.  Test infrastructure only."""
import re

import bammodel
import moltagmodel as mm
from moltagmodel import Stop


def attributes(aux):
    """aux bytes -> {tag str: (type char, value)}; a Z value is its bytes, any other type None; a repeated tag keeps its last value"""
    out = {}
    p, n = 0, len(aux)
    while p < n:
        tag, ty = aux[p:p + 2].decode("latin-1"), chr(aux[p + 2])
        v = p + 3
        if ty in mm._W:
            q = v + mm._W[ty]
        elif ty in "ZH":
            q = aux.index(b"\0", v) + 1
        elif ty == "B":
            q = v + 5 + mm._W[chr(aux[v])] * int.from_bytes(aux[v + 1:v + 5], "little")
        else:
            raise mm.BadAux("type")
        out[tag] = (ty, aux[v:q - 1] if ty == "Z" else None)
        p = q
    return out


def java_regex_split(s, pattern):
    """String.split(regex): a leading empty piece stays when the match at 0 is not empty, trailing empty pieces go; no match -> [s]"""
    parts = re.split(pattern, s)
    while len(parts) > 1 and parts[-1] == "":
        parts.pop()
    if parts == [""] and s != "":
        return []
    return parts


def cigar_string(cigar):
    """SAMRecord.getCigarString"""
    return "".join(f"{n}{op}" for op, n in cigar) if cigar else "*"


def _string(attrs, tag):
    """(String) r.getAttribute(tag): None when missing, TypeError where the cast throws"""
    if tag not in attrs:
        return None
    ty, v = attrs[tag]
    if ty != "Z":
        raise TypeError(tag)
    return v


def export_clipped_reads(bam, min_clip=150, cell_tag="BC", umi_tag="U8", gene_tag="GE", us_tag="US", qs_tag="QS"):
    """-> (FASTQ bytes, dict(records, clipped, written), [(clipped, written) per record]); raises Stop(read, record) where the reference's
    loop dies"""
    _text, _refs, recs = bammodel.parse_bam(bam)
    out, seen, decisions = [], set(), []
    counts = dict(records=0, clipped=0, written=0)
    for i, r in enumerate(recs):
        try:
            counts["records"] += 1                                                  # L66
            tmp = mm.java_split(r["name"], "_")                                     # L68
            attrs = attributes(r["aux"])
            gene, cell, umi = _string(attrs, gene_tag), _string(attrs, cell_tag), _string(attrs, umi_tag)      # L72-74
            key = b"_".join([tmp[0].encode("latin-1")] + [b"null" if v is None else v for v in (gene, cell, umi)])  # L76 (IndexError: no piece)
            cigar = cigar_string(r["cigar"])                                        # L78
            ctype = java_regex_split(cigar, "[0-9]+")                               # L79
            csize = java_regex_split(cigar, "[A-Z]")                                # L80
            clipped = False
            if ctype[1] in ("H", "S") and int(csize[0]) > min_clip:                 # L82 (IndexError: "*"; ValueError: NumberFormatException)
                clipped = True
            if ctype[-1] in ("H", "S") and int(csize[-1]) > min_clip:               # L84
                clipped = True
            wrote = False
            if clipped and key not in seen:                                         # L87
                us, qs = _string(attrs, us_tag), _string(attrs, qs_tag)             # L91-92
                out.append(b"@" + key + b"\n" + (b"null" if us is None else us) + b"\n+\n" + (b"null" if qs is None else qs) + b"\n")   # L93
                seen.add(key)                                                       # L94
                wrote = True
            counts["clipped"] += clipped
            counts["written"] += wrote
            decisions.append((clipped, wrote))
        except (IndexError, ValueError, TypeError):
            raise Stop(r["name"], i) from None
    return b"".join(out), counts, decisions


def read_edits(name, gene="GE", cell="BC", umi="U8"):
    """AddBamReadTags.java:L49-62 -> edits in call order"""
    info = mm.java_split(name, "_")
    if len(info) == 3:
        return [(gene, info[0]), (cell, info[1]), (umi, info[2])]
    if len(info) == 4:
        return [(gene, info[1]), (cell, info[2]), (umi, info[3])]
    return []


def add_bam_read_tags(bam, gene="GE", cell="BC", umi="U8"):
    """-> (inflated output BAM, dict(records, tagged))"""
    cnt = dict(records=0, tagged=0)

    def decide(_i, r):
        e = read_edits(r["name"], gene, cell, umi)
        cnt["records"] += 1
        cnt["tagged"] += bool(e)
        return e
    return mm.rewrite(bam, lambda h: h, decide), cnt
