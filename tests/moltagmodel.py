"""Plain-Python model of `AddBamMoleculeTags` (AddBamMoleculeTags.java:L38-67) and `AddGeneNameTag` (AddGeneNameTag.java:L76-395) over an
inflated BAM: every record as the reference writes it, the counters, and the record on which its loop dies.  Gene model, alignment blocks
and the order of a multi-gene value come from tests/genemodel.py, record bytes from tests/bammodel.py; the attribute list below follows
the rule tests/golden/ref_exec_auxorder.json pins.  Test infrastructure only."""
import struct

import numpy as np

import bammodel
import genemodel as gm
from pymodel import JHashSet

MAX_FIELDS = 64      # SMI_TAGBAM_MAX_ATTRS


class Stop(Exception):
    """the reference's loop ends at this record (an exception its catch swallows): .read, .record"""

    def __init__(self, read, record):
        super().__init__(read)
        self.read, self.record = read, record


class BadAux(Exception):
    pass


# ---- the attribute list ------------------------------------------------------------------------------------------------------------------
_W = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


def int_field(v):
    """BinaryTagCodec.getIntegerType: the smallest type that holds v, signed first"""
    for code, lo, hi in (("c", -128, 127), ("C", 0, 255), ("s", -32768, 32767), ("S", 0, 65535), ("i", -2 ** 31, 2 ** 31 - 1), ("I", 0, 2 ** 32 - 1)):
        if lo <= v <= hi:
            return code.encode() + struct.pack(_INT[code], v)
    raise BadAux("integer out of range")


def read_aux(aux):
    """aux bytes -> {tag bytes: value bytes (type byte on) as htsjdk writes it back}: a repeated tag keeps its last value, integers are
    re-typed, H becomes B:c"""
    cur, p, n = {}, 0, len(aux)
    while p < n:
        if p + 3 > n:
            raise BadAux("cut off")
        tag, ty = aux[p:p + 2], chr(aux[p + 2])
        v = p + 3
        if ty in _W:
            q = v + _W[ty]
            if q > n:
                raise BadAux("cut off")
            val = int_field(struct.unpack(_INT[ty], aux[v:q])[0]) if ty in _INT else aux[p + 2:q]
        elif ty in "ZH":
            q = aux.find(b"\0", v)
            if q < 0:
                raise BadAux("no NUL")
            if ty == "H":
                digits = aux[v:q].decode("latin-1")
                if len(digits) % 2 or any(c not in "0123456789abcdefABCDEF" for c in digits):
                    raise BadAux("hex")
                val = b"Bc" + struct.pack("<I", len(digits) // 2) + bytes.fromhex(digits)
            else:
                val = aux[p + 2:q + 1]
            q += 1
        elif ty == "B":
            if v + 5 > n or chr(aux[v]) not in "cCsSiIf":
                raise BadAux("array")
            q = v + 5 + _W[chr(aux[v])] * struct.unpack_from("<I", aux, v + 1)[0]
            if q > n:
                raise BadAux("cut off")
            val = aux[p + 2:q]
        else:
            raise BadAux("type")
        if tag not in cur and len(cur) >= MAX_FIELDS:
            raise BadAux("too many")
        cur[tag] = bytes(val)
        p = q
    return cur


def edit_aux(aux, edits):
    """edits: [(tag str, str | int | None)] in call order (SAMRecord.setAttribute; None removes) -> the attribute bytes as written"""
    cur = read_aux(aux)
    for tag, value in edits:
        t = tag.encode("latin-1")
        if value is None:
            cur.pop(t, None)
            continue
        if t not in cur and len(cur) >= MAX_FIELDS:
            raise BadAux("too many")
        cur[t] = int_field(value) if isinstance(value, int) else b"Z" + value.encode("latin-1") + b"\0"
    return b"".join(t + v for t, v in sorted(cur.items(), key=lambda kv: kv[0][1] << 8 | kv[0][0]))


def rewrite(bam, header, decide):
    """every record of the inflated BAM through decide(index, parsed record) -> edits; header: bytes -> bytes"""
    _text, _refs, recs = bammodel.parse_bam(bam)
    start = recs[0]["off"] if recs else len(bam)
    out = [header(bam[:start])]
    for i, r in enumerate(recs):
        raw = bam[r["off"] + 4:r["off"] + r["length"]]
        fixed = raw[:len(raw) - len(r["aux"])]
        body = fixed + edit_aux(r["aux"], decide(i, r))
        out.append(struct.pack("<I", len(body)) + body)
    return b"".join(out)


# ---- AddBamMoleculeTags ------------------------------------------------------------------------------------------------------------------
def java_split(s, sep):
    """String.split(sep) for one literal character: trailing empty pieces dropped, leading and inner ones kept; "" -> [""]"""
    if s == "":
        return [""]
    parts = s.split(sep)
    while parts and parts[-1] == "":
        parts.pop()
    return parts


def java_int(s):
    """new Integer(s): optional sign, decimal digits, the int range; None = NumberFormatException"""
    body = s[1:] if s[:1] in ("+", "-") else s
    if not body or any(c not in "0123456789" for c in body):
        return None
    v = int(body) * (-1 if s[0] == "-" else 1)
    return v if -2 ** 31 <= v <= 2 ** 31 - 1 else None


def name_edits(name, cell="BC", umi="U8", rn="RN"):
    """-> edits, or raises ValueError where Integer throws"""
    info = java_split(name, "-")
    if len(info) == 1:
        info = java_split(name, "|")
    if len(info) != 3:
        return []
    v = java_int(info[2])
    if v is None:
        raise ValueError(name)
    return [(cell, info[0]), (umi, info[1]), (rn, v)]


def add_molecule_tags(bam, cell="BC", umi="U8", rn="RN"):
    """-> (inflated output BAM, counts); raises Stop at the first read whose third piece is no int"""
    counts = dict(records=0, tagged=0)

    def decide(i, r):
        try:
            e = name_edits(r["name"], cell, umi, rn)
        except ValueError:
            raise Stop(r["name"], i)
        counts["records"] += 1
        counts["tagged"] += bool(e)
        return e

    return rewrite(bam, lambda h: h, decide), counts


# ---- AddGeneNameTag ----------------------------------------------------------------------------------------------------------------------
class GeneModel:
    def __init__(self, refflat_text, ref_names):
        self.tree, self.n_genes = gm.load_refflat(refflat_text, ref_names)
        self.refs = list(ref_names)
        self._lf = {}

    def locus(self, g):
        """per base of [g.start, g.end] the maximum over the gene's transcripts of what assignLocusFunctionForRange assigns (Gene.java:L151-165),
        painted into one array of bases; positions outside are INTERGENIC"""
        a = self._lf.get(id(g))
        if a is None:
            a = np.zeros(g.end - g.start + 1, dtype=np.uint8)

            def paint(lo, hi, f):                     # a[p] = max(a[p], f) for every base p of [lo, hi]
                if lo <= hi:
                    np.maximum(a[lo - g.start:hi - g.start + 1], f, out=a[lo - g.start:hi - g.start + 1])

            for t in g.transcripts():
                lo, hi = max(t["tx"][0], g.start), min(t["tx"][1], g.end)
                paint(lo, hi, gm.INTRONIC)
                for s, e in t["exons"]:
                    s, e = max(s, lo), min(e, hi)
                    paint(s, e, gm.UTR)                                   # utr(locus): locus < cdsStart or locus > cdsEnd ...
                    paint(max(s, t["cds"][0]), min(e, t["cds"][1]), gm.CODING)   # ... every other exon base is CODING
            self._lf[id(g)] = a
        return a

    def block_function(self, g, bs, bl):
        a = self.locus(g)
        lo, hi = max(bs, g.start), min(bs + bl - 1, g.end)
        return int(a[lo - g.start:hi - g.start + 1].max()) if lo <= hi else gm.INTERGENIC


def gene_decision(model, contig, flag, pos0, cigar, use_strand=True, allow_multi=True):
    """setGeneExons (L116-160) for one record -> dict(xf, genes [Gene in value order], same, opposite) or None for an unmapped record;
    raises ValueError where getLocusFunction meets a null (L362)"""
    if flag & 4 or contig is None:
        return None
    blocks, end = gm.blocks_of(pos0 + 1, cigar)
    over = JHashSet()                                             # getOverlaps L267: [start, end] against the tree's nodes, no guard
    for (s, e), node in model.tree.get(contig, []):
        if s <= end and e >= pos0 + 1:
            for g in node:
                over.add(g.hash(), g.key(), g)
    fmap = gm.JMap()
    for g in over:                                                # L269-272
        if not blocks:
            raise ValueError("null locus function")
        fmap.put(g.hash(), g.key(), (g, gm.top([model.block_function(g, bs, bl) for bs, bl in blocks])))
    keys = [g for _, (g, _) in fmap.items()]
    result = JHashSet()                                           # getConsistentExons L196-217
    for bs, bl in blocks:
        bg = JHashSet()
        for g in keys:
            if any(s <= bs + bl - 1 and bs <= e for t in g.transcripts() for s, e in t["exons"]):
                bg.add(g.hash(), g.key(), g)
        if bg.size and allow_multi:                               # retainAll on a set that starts empty keeps it empty
            for g in bg:
                result.add(g.hash(), g.key(), g)
    genes = [g for g in result if fmap.get(g.key())[1] in (gm.CODING, gm.UTR)]
    xf = gm.INTERGENIC if len(fmap) == 0 else gm.top([v for _, (_, v) in fmap.items()])
    neg = bool(flag & 16)
    same = [g for g in genes if g.negative == neg]
    opposite = [g for g in genes if g.negative != neg]
    kept = genes
    if use_strand:                                                # getGenesConsistentWithReadStrand L162-194
        kept = [] if (not same and opposite) else same
    return dict(xf=xf, genes=kept, same=len(same), opposite=len(opposite))


def gene_edits(d, gene_tag="GE", strand_tag="GS", fn_tag="XF"):
    if d is None:
        return []
    e = [(fn_tag, gm.NAMES[d["xf"]])]
    if d["genes"]:
        return e + [(gene_tag, ",".join(g.name for g in d["genes"])), (strand_tag, ",".join("-" if g.negative else "+" for g in d["genes"]))]
    return e + [(gene_tag, None), (strand_tag, None)]


def unsorted_header(hdr):
    """samFileHeader.setSortOrder(unsorted) as this build writes it"""
    l_text = struct.unpack_from("<I", hdr, 4)[0]
    lines = hdr[8:8 + l_text].decode("latin-1").split("\n")
    if lines and lines[0].startswith("@HD"):
        f = lines[0].split("\t")
        so = [i for i in range(1, len(f)) if f[i].startswith("SO:")]
        if so:
            f[so[0]] = "SO:unsorted"
        else:
            f.append("SO:unsorted")
        lines[0] = "\t".join(f)
        text = "\n".join(lines)
    else:
        text = "@HD\tVN:1.6\tSO:unsorted\n" + "\n".join(lines)
    t = text.encode("latin-1")
    return b"BAM\1" + struct.pack("<I", len(t)) + t + hdr[8 + l_text:]


def add_gene_name_tag(bam, refflat_text, gene_tag="GE", strand_tag="GS", fn_tag="XF", use_strand=True, allow_multi=True, model=None):
    """-> (inflated output BAM, counts, [decision per record]); raises Stop at the first mapped record without a block under a gene"""
    _text, refs, _recs = bammodel.parse_bam(bam[:bammodel_records_start(bam)])
    names = [r[0] for r in refs]
    model = model or GeneModel(refflat_text, names)
    c = dict(records=0, tagged=0, total_reads=0, wrong_strand=0, right_strand=0, ambiguous_fixed=0, ambiguous_rejected=0, multi_gene_records=0,
             with_gene=0, genes=model.n_genes)
    decisions = []

    def decide(i, r):
        contig = names[r["ref_id"]] if 0 <= r["ref_id"] < len(names) else None
        try:
            d = gene_decision(model, contig, r["flag"], r["pos0"], r["cigar"], use_strand, allow_multi)
        except ValueError:
            raise Stop(r["name"], i)
        decisions.append(d)
        c["records"] += 1
        if d is not None:
            c["tagged"] += 1
            c["with_gene"] += bool(d["genes"])
            c["multi_gene_records"] += len(d["genes"]) > 1
            if use_strand:                                        # L164-193
                c["total_reads"] += 1
                if not d["same"] and d["opposite"]:
                    c["wrong_strand"] += 1
                else:
                    c["ambiguous_fixed"] += d["opposite"] > 0
                    c["right_strand"] += 1
        return gene_edits(d, gene_tag, strand_tag, fn_tag)

    return rewrite(bam, unsorted_header, decide), c, decisions


def bammodel_records_start(bam):
    l_text = struct.unpack_from("<I", bam, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<I", bam, p)[0]
    p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<I", bam, p)[0]
    return p


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
def refflat_line(gene, tx, chrom, strand, tx_start, tx_end, cds_start, cds_end, exons):
    """coordinates 1-based inclusive as the model keeps them -> one refFlat line (0-based starts)"""
    return "\t".join([gene, tx, chrom, strand, str(tx_start - 1), str(tx_end), str(cds_start - 1), str(cds_end), str(len(exons)),
                      ",".join(str(s - 1) for s, _ in exons) + ",", ",".join(str(e) for _, e in exons) + ","])
