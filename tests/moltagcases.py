"""The hand-built inputs of tests/test_moltag_cpu.py and tests/test_moltag_gpu.py: refFlat texts, reference lists and BAM records for every
shape the AddBamMoleculeTags / AddGeneNameTag issue lists.  Test infrastructure only."""
import random

import bammodel
import tagbammodel as tm
from moltagmodel import refflat_line as L

HEAD = "@HD\tVN:1.6\tSO:coordinate\n"
QUERY_OPS = "M=XIS"


def rec(name, cigar, pos1=1, ref=0, flag=0, aux=b""):
    """pos1: 1-based alignment start; the sequence is as long as the CIGAR says"""
    n = sum(ln for op, ln in cigar if op in QUERY_OPS)
    return bammodel.bam_record(name, flag, ref, pos1 - 1, 60, cigar, "A" * n, aux=aux)


def bam_of(refs, records, head=HEAD):
    return bammodel.bam_bytes(head + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs), refs, records)


# ---- names (AddBamMoleculeTags) ----------------------------------------------------------------------------------------------------------
LONG_NAME = "C" * 120 + "-" + "G" * 125 + "-" + "1234567"          # 254 bytes
NAMES = ["A-B-3", "A-B-3-", "-B-3", "A--3", "A-B-3-4", "A-B", "A-", "-", "*", "A|B|3", "A|B|3|", "A|B-3", "|", LONG_NAME, "ACGT-TTTT-007", "ACGT-TTTT-+7",
         "ACGT-TTTT--5", "", "--", "||", "A|B", "-|-", "a-b-3--", "A|B|3||", "|B|3"]
NAMES += [f"ACGTACGTACGTACGT-TTTTGGGGCCCC-{v}" for v in (0, 127, 128, 255, 256, 32767, 32768, 65535, 65536, 2147483647, -128, -129, -32768, -32769,
                                                          -2147483648)]
# third pieces Integer refuses.  A negative number cannot BE a third piece: its '-' is a separator ("A-B--5" has four pieces, "A|B|-5" two),
# so the sign branch is reached by '+' only and by the lone "-" of "A|B|-" (one piece at '-', three at '|')
STOP_NAMES = [f"ACGT-TTTT-{v}" for v in ("2147483648", " 3", "3x", "+", "3 ", "99999999999999999999")] + ["A|B|-", "A|B|", "A|B|x"][::2]
assert len(LONG_NAME) == 254


def name_records():
    aux = [b"", tm.aux_int("BC", "i", 5) + tm.aux_z("U8", "old") + tm.aux_z("RN", "text"),                       # other types replaced
           tm.aux_z("AA", "x") + tm.aux_z("BB", "x") + tm.aux_z("BD", "x") + tm.aux_z("T8", "x") + tm.aux_z("V8", "x") + tm.aux_z("QN", "x")
           + tm.aux_z("SN", "x") + tm.aux_z("U7", "x") + tm.aux_z("U9", "x") + tm.aux_z("RM", "x") + tm.aux_z("RO", "x"),   # both sides of each tag
           tm.aux_h("XH", "0aFF") + tm.aux_b("XB", "s", [1, -2, 3]) + tm.aux_int("RN", "I", 70000) + tm.aux_int("NM", "i", 2) + tm.aux_z("RN", "dup")]
    out = []
    for k, nm in enumerate(NAMES):
        unmapped = k % 5 == 4
        out.append(rec(nm, [("M", 8)], pos1=10 + k, ref=-1 if unmapped else 0, flag=4 if unmapped else 0, aux=aux[k % len(aux)]))
    return out


def many_attrs(n):
    return b"".join(tm.aux_int("%c%c" % (ord("a") + k // 26, ord("a") + k % 26), "C", k) for k in range(n))


# ---- genes -------------------------------------------------------------------------------------------------------------------------------
def search_case():
    """records under 0, 1, 63, 64, 65 and 200 genes (one contig each), inclusive borders, a wide gene in front of 400 short ones, a contig
    without genes, flag 4 with a reference id"""
    counts = [0, 1, 63, 64, 65, 200]
    refs = [(f"n{c}", 100000) for c in counts] + [("border", 100000), ("wide", 200000), ("empty", 100000)]
    lines, records = [], []
    for ci, c in enumerate(counts):
        for k in range(c):      # nested genes, alternating strands, one exon each, half of them non-coding
            s, e = 5000 - 3 * k, 6000 + 7 * k
            lines.append(L(f"G{c}_{k}", f"T{c}_{k}", f"n{c}", "+-"[k % 2], s, e, s + 10 if k % 4 < 2 else e + 1, e - 10 if k % 4 < 2 else e, [(s, e)]))
        records += [rec(f"under{c}", [("M", 50)], 5500, ci), rec(f"under{c}r", [("M", 20), ("N", 30), ("M", 20)], 5500, ci, flag=16)]
    b = len(counts)
    lines.append(L("BORD", "TB", "border", "+", 1000, 2000, 1100, 1900, [(1000, 1200), (1800, 2000)]))
    for nm, cg, p in (("endin", [("M", 10)], 991), ("endout", [("M", 10)], 990), ("startin", [("M", 10)], 2000), ("startout", [("M", 10)], 2001),
                      ("delin", [("M", 5), ("D", 6)], 990), ("skipin", [("M", 5), ("N", 6)], 989), ("skipout", [("M", 5), ("N", 5)], 989)):
        records.append(rec(nm, cg, p, b))
    lines.append(L("WIDE", "TW", "wide", "+", 100, 150000, 100, 150000, [(100, 200), (149000, 150000)]))
    for k in range(400):
        s = 1000 + 100 * k
        lines.append(L(f"S{k}", f"TS{k}", "wide", "+", s, s + 50, s, s + 50, [(s, s + 50)]))
    records += [rec("widefar", [("M", 30)], 149500, b + 1), rec("widelast", [("M", 30)], 1000 + 100 * 399 + 10, b + 1), rec("widemid", [("M", 30)], 60000, b + 1),
                rec("nogenes", [("M", 30)], 5000, b + 2), rec("flag4", [("M", 50)], 5500, 1, flag=4, aux=tm.aux_z("GE", "old") + tm.aux_z("GS", "+")),
                rec("noref", [("M", 50)], 0, -1, flag=4, aux=tm.aux_z("GE", "old")),
                rec("stale", [("M", 30)], 5000, b + 2, aux=tm.aux_z("GE", "old") + tm.aux_z("GS", "-") + tm.aux_int("XF", "C", 3) + tm.aux_h("XH", "00ff"))]
    return "\n".join(lines) + "\n", refs, records


def _exons(n, start, width=10, gap=10):
    return [(start + k * (width + gap), start + k * (width + gap) + width - 1) for k in range(n)]


def locus_case():
    refs = [("chrT", 10 ** 6), ("chrE", 10 ** 6), ("chrF", 10 ** 6)]
    lines, records = [], []
    for n in (1, 63, 64, 65, 200):      # genes of n transcripts: only the LAST one (in file order) has its exon under the read
        base = 10000 * (1 + [1, 63, 64, 65, 200].index(n))
        for k in range(n):
            ex = [(base + 500, base + 520)] if k == n - 1 else [(base + 10 * (k % 20), base + 10 * (k % 20) + 5)]
            lines.append(L(f"GT{n}", f"GT{n}_t{k}", "chrT", "+", base, base + 1000 + k, base + 505, base + 510, ex))
        records += [rec(f"tx{n}_coding", [("M", 4)], base + 504, 0), rec(f"tx{n}_utr", [("M", 4)], base + 512, 0),
                    rec(f"tx{n}_intron", [("M", 4)], base + 700, 0)]
    for n in (1, 63, 64, 65, 300):      # transcripts of n exons; reads on the first, the last and between
        base = 20000 * (1 + [1, 63, 64, 65, 300].index(n))
        ex = _exons(n, base)
        lines.append(L(f"GE{n}", f"GE{n}_t", "chrE", "-", base, ex[-1][1], ex[0][0] + 3, ex[-1][1] - 3, ex))
        for nm, p, ln in (("first", ex[0][0], 3), ("last", ex[-1][1] - 2, 3), ("mid", ex[n // 2][0] + 2, 4), ("span", ex[0][0], ex[-1][1] - ex[0][0] + 1)):
            records.append(rec(f"ex{n}_{nm}", [("M", ln)], p, 1, flag=16))
        if n > 1:
            records.append(rec(f"ex{n}_gap", [("M", 4)], ex[n // 2 - 1][1] + 2, 1, flag=16))
    # one base on either side of an exon and of the CDS; a non-coding line; intron only; between two transcripts; coding for one, intronic for another
    lines += [L("F1", "F1a", "chrF", "+", 1000, 3000, 1150, 2850, [(1100, 1200), (2800, 2900)]),
              L("NC", "NCa", "chrF", "+", 5000, 6000, 6001, 6000, [(5000, 5100), (5900, 6000)]),
              L("TWO", "TWOa", "chrF", "+", 8000, 8100, 8000, 8100, [(8000, 8100)]), L("TWO", "TWOb", "chrF", "+", 8500, 8600, 8500, 8600, [(8500, 8600)]),
              L("OUT", "OUTa", "chrF", "+", 12000, 12100, 12000, 12100, [(11950, 12050), (12080, 12150)]),   # exons reaching outside the transcript
              L("BIG", "BIGa", "chrF", "+", 20000, 30000, 20000, 30000, [(20000, 20100), (29900, 30000)]),
              L("SMALL", "SMALLa", "chrF", "+", 25000, 25100, 25010, 25090, [(25000, 25100)])]
    for nm, p, ln in (("touchL", 1090, 11), ("missL", 1090, 10), ("touchR", 1200, 5), ("missR", 1201, 5), ("cdsL_hit", 1145, 6), ("cdsL_miss", 1145, 5),
                      ("cdsR_hit", 2850, 5), ("cdsR_miss", 2851, 5), ("cds_in", 1160, 5), ("nc_exon", 5050, 10), ("nc_intron", 5500, 10),
                      ("intron", 2000, 50), ("between", 8200, 100), ("two_a", 8050, 10), ("out_l", 11960, 20), ("out_in", 11990, 20), ("out_r", 12120, 20),
                      ("both", 25020, 10), ("both_utr", 25000, 5), ("before", 900, 50), ("cover", 900, 2500)):
        records.append(rec(nm, [("M", ln)], p, 2))
    records.append(rec("split", [("M", 10), ("N", 1590), ("M", 10)], 1195, 2))
    records.append(rec("out_split", [("M", 10), ("N", 50), ("M", 10)], 12060, 2))     # an exon hit outside the transcript, INTRONIC inside
    return "\n".join(lines) + "\n", refs, records


def _cigar(n, seed):
    rnd = random.Random(seed)
    ops = [("S", 2)] + [("M=XIDNP"[rnd.randrange(7)], rnd.randrange(1, 4)) for _ in range(n - 2)] + [("H", 3)] if n >= 3 else [("M", 5)] * n
    return ops


def cigar_case():
    refs = [("chrC", 10 ** 6)]
    lines = [L("CG", "CGa", "chrC", "+", 1000, 5000, 1100, 1500, _exons(150, 1000, 7, 6)), L("CR", "CRa", "chrC", "-", 1300, 1400, 1300, 1400, [(1300, 1400)])]
    records = []
    for n in (1, 63, 64, 65, 127, 128, 129, 300):
        for k in range(3):
            records.append(rec(f"cig{n}_{k}", _cigar(n, 100 * n + k), 990 + 37 * k, 0, flag=16 * (k == 2)))
    # blocks on the first and the last operation of a round only
    fill = [("N", 3), ("I", 1)] * 31
    records.append(rec("round0", [("M", 4)] + fill + [("M", 4)], 1001, 0))
    records.append(rec("round1", [("N", 2)] * 64 + [("M", 4)] + fill + [("M", 4)], 1001, 0))
    records.append(rec("round1only", [("N", 2), ("P", 1)] * 32 + [("N", 1)] * 63 + [("X", 4)], 1001, 0))
    return "\n".join(lines) + "\n", refs, records


def strand_case():
    """same strand only / opposite only / both; two and three same-strand genes"""
    refs = [("chrS", 10 ** 6)]
    lines = [L("P1", "P1a", "chrS", "+", 1000, 2000, 1000, 2000, [(1000, 2000)]), L("M1", "M1a", "chrS", "-", 3000, 4000, 3000, 4000, [(3000, 4000)]),
             L("P2", "P2a", "chrS", "+", 5000, 6000, 5000, 6000, [(5000, 6000)]), L("M2", "M2a", "chrS", "-", 5500, 6500, 5500, 6500, [(5500, 6500)]),
             L("D1", "D1a", "chrS", "+", 8000, 9000, 8000, 9000, [(8000, 9000)]), L("D2", "D2a", "chrS", "+", 8100, 9100, 8100, 9100, [(8100, 9100)]),
             L("D3", "D3a", "chrS", "+", 8200, 9200, 8200, 9200, [(8200, 9200)]), L("D4", "D4a", "chrS", "-", 8300, 9300, 8300, 9300, [(8300, 9300)])]
    old = tm.aux_z("GE", "old") + tm.aux_z("GS", "?") + tm.aux_z("ZZ", "keep")
    records = [rec("same", [("M", 50)], 1500, 0, aux=old), rec("opposite", [("M", 50)], 3500, 0, aux=old), rec("opposite_r", [("M", 50)], 1500, 0, flag=16),
               rec("both", [("M", 50)], 5700, 0), rec("both_r", [("M", 50)], 5700, 0, flag=16), rec("two", [("M", 50)], 8120, 0),
               rec("three", [("M", 50)], 8250, 0), rec("three_and_opp", [("M", 50)], 8400, 0), rec("three_r", [("M", 50)], 8400, 0, flag=16),
               rec("none", [("M", 50)], 20000, 0, aux=old), rec("three_blocks", [("M", 10), ("N", 100), ("M", 10), ("N", 100), ("M", 10)], 7950, 0)]
    return "\n".join(lines) + "\n", refs, records


def collision_pair(contig="chrH"):
    """two '+' genes on one contig whose Interval.hashCode values fall into one bucket of a 16-slot table, picked with the model's hash"""
    import genemodel as gm

    def bucket(s, e):
        h = gm.Gene(contig, s, e, False, "x").hash()
        return (h ^ (h >> 16)) & 15

    a = (1000, 2000)
    for s in range(1001, 1100):
        for e in range(2001, 2100):
            if bucket(s, e) == bucket(*a):
                return a, (s, e)
    raise AssertionError("no colliding pair")


def collision_case():
    a, b = collision_pair()
    refs = [("chrH", 10 ** 6)]
    lines = [L("HB", "HBa", "chrH", "+", b[0], b[1], b[0], b[1], [b]), L("HA", "HAa", "chrH", "+", a[0], a[1], a[0], a[1], [a]),
             L("HC", "HCa", "chrH", "+", 1200, 2500, 1200, 2500, [(1200, 2500)])]
    records = [rec("pair", [("M", 50)], 1100, 0), rec("trio", [("M", 50)], 1500, 0)]
    return "\n".join(lines) + "\n", refs, records, (a, b)


def error_case(under_gene):
    refs = [("chrS", 10 ** 6)]
    lines = [L("P1", "P1a", "chrS", "+", 1000, 2000, 1000, 2000, [(1000, 2000)])]
    records = [rec("fine0", [("M", 50)], 1500, 0), rec("clipped", [("S", 10)], 1500 if under_gene else 5000, 0), rec("fine1", [("M", 50)], 1500, 0),
               rec("clipped2", [("S", 10)], 1600 if under_gene else 5000, 0)]
    return "\n".join(lines) + "\n", refs, records


GENE_CASES = {"search": search_case, "locus": locus_case, "cigar": cigar_case, "strand": strand_case, "collision": lambda: collision_case()[:3]}


def damaged_records():
    """name -> a record whose attributes no walker accepts (tests/auxcases.py DAMAGED), for K-EDIT's clean refusal"""
    import auxcases
    return {k: rec("plain", [("M", 4)], aux=tm.aux_z("XA", "a") + v) for k, v in auxcases.DAMAGED.items()}
