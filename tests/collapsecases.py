"""Inputs of the CollapseModel tests (test infrastructure only), built from literals and seeds: the hand-built case whose outputs
tests/test_collapse_cpu.py spells out, and the generators of the size, threshold and order edges tests/test_collapse_gpu.py runs (each edge
is asserted present with the model in test_collapse_cpu.py)."""
import numpy as np

import bammodel
import tagbammodel as tm

HEAD = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr12\tLN:2000000\n@SQ\tSN:chrB\tLN:2000000\n"
REFS = [("chr12", 2000000), ("chrB", 2000000)]
BLOCK = 256      # threads of one K-COLLAPSE block
LDS_JUNC = 1024  # junctions K-COLLAPSE stages in LDS


def cigar_for(junc, pos1, tail=30):
    """M / N operations whose junctions are `junc` ((exon end, next exon start) pairs) -> (pos0, cigar)"""
    cig, cur = [], pos1
    for e, s in junc:
        cig.append(("M", e - cur + 1))
        cig.append(("N", s - e - 1))
        cur = s
    cig.append(("M", tail))
    assert all(n > 0 for _o, n in cig), (junc, pos1)
    return pos1 - 1, cig


def rec(name, junc, gene, it="undef", bc="CELL1", start=None, flag=0, mapq=60, rn=None, ref_id=0, cigar=None, umi="U", extra=b""):
    start = (junc[0][0] - 100 if junc else 1000) if start is None else start
    pos0, cig = cigar_for(junc, start)
    aux = b""
    if bc is not None:
        aux += tm.aux_z("BC", bc)
    if umi is not None:
        aux += tm.aux_z("U8", umi)
    if gene is not None:
        aux += tm.aux_z("IG", gene)
    if it is not None:
        aux += tm.aux_z("IT", it)
    if rn is not None:
        aux += tm.aux_int("RN", "C", rn)
    return bammodel.bam_record(name, flag, ref_id, pos0, mapq, cigar or cig, "ACGT", aux=aux + extra)


# ---- the hand-built case ---------------------------------------------------------------------------------------------------------------
# GA: TA1 (1100-2001, 2100-3001), TA2 (1100-3001), TA3 (1100-1501, 1600-2001, 2100-3001; never evidenced), TA4 (4100-5001); GB: TB1 (three
# junctions), TB2 (1100-3001); GZ: a line without exon bases (not in the model)
HAND_REF = ("GA\tTA1\tchr12\t+\t999\t3100\t1050\t3050\t3\t999,2000,3000,\t1100,2100,3100,\n"
            "GA\tTA2\tchr12\t+\t999\t3100\t999\t3100\t2\t999,3000,\t1100,3100,\n"
            "GA\tTA3\tchr12\t+\t999\t3100\t999\t3100\t4\t999,1500,2000,3000,\t1100,1600,2100,3100,\n"
            "GA\tTA4\tchr12\t+\t3999\t5100\t3999\t5100\t2\t3999,5000,\t4100,5100,\n"
            "GB\tTB1\tchr12\t+\t999\t4100\t999\t4100\t4\t999,2000,3000,4000,\t1100,2100,3100,4100,\n"
            "GB\tTB2\tchr12\t+\t999\t3100\t999\t3100\t2\t999,3000,\t1100,3100,\n"
            "GZ\tTZ0\tchr12\t+\t10\t10\t10\t10\t1\t10,\t10,\n")
HAND_CSV = "CELL1-1\nCELL2\nCELL3\n"
# a refFlat line the parser fails on: {case: (line number, the line that stands there instead of HAND_REF's)}
BAD_REF_LINES = dict(
    short=(3, "GA\tTA3\tchr12\t+\t999\t3100\t999\t3100\t4\t999,1500,2000,3000,"),                       # ten fields
    strand=(2, "GA\tTA2\tchr12\tx\t999\t3100\t999\t3100\t2\t999,3000,\t1100,3100,"),
    integer=(5, "GB\tTB1\tchr12\t+\t999\t41o0\t999\t4100\t4\t999,2000,3000,4000,\t1100,2100,3100,4100,"),
    in_list=(6, "GB\tTB2\tchr12\t+\t999\t3100\t999\t3100\t2\t999,3000,\t1100,31x0,"),
    ends=(1, "GA\tTA1\tchr12\t+\t999\t3100\t1050\t3050\t3\t999,2000,3000,\t1100,2100,"))                 # three exon starts, two ends


def bad_refflat(which):
    no, bad = BAD_REF_LINES[which]
    lines = HAND_REF.split("\n")
    lines[no - 1] = bad
    return "\n".join(lines)
TA1 = [(1100, 2001), (2100, 3001)]
TB1 = [(1100, 2001), (2100, 3001), (3100, 4001)]


def hand_records(order_gc2=("b", "a", "c")):
    R = []
    # the loader's filter: none of these is evidence
    R += [rec("f_nobc", TA1, "GA", "TA1", bc=None), rec("f_unmapped", TA1, "GA", "TA1", flag=4), rec("f_mapq0", TA1, "GA", "TA1", mapq=0)]
    p, c = cigar_for(TA1, 1000)
    R += [rec("f_chim", TA1, "GA", "TA1", cigar=[("S", 151)] + c), rec("f_lowrn", TA1, "GA", "TA1", rn=0), rec("f_notlisted", TA1, "GA", "TA1", bc="CELLX")]
    R += [rec("f_minus1", TA1, "GA", "TA1", bc="CELL1-1"), rec("f_nogene", TA1, None, "TA1"), rec("f_emptygene", TA1, "", "undef")]
    R += [rec("f_undefgene", TA1, "undef", "undef")]
    R += [rec("o1", [(102, 500)], "GO", ref_id=1, start=50, flag=16)]       # GO: in front of o2 in the file, behind it in the dictionary
    # GA
    R += [rec("a_known1", TA1, "GA", "TA1", start=1000), rec("a_known2", TA1, "GA", "TA1", bc="CELL2", start=1000, rn=3)]
    R += [rec("a_mono", [], "GA")]
    R += [rec(f"a_ckj{i}", [(1100, 3001), (4100, 5001)], "GA", start=1000) for i in range(2)]
    R += [rec(f"a_cks{i}", [(1100, 5001)], "GA", bc=f"CELL{i + 1}", start=1000) for i in range(2)]
    R += [rec("a_single", [(1100, 2700)], "GA", start=1000)]                 # one record: Novel.3 is never printed
    R += [rec("a_nss0", [(1100, 2500)], "GA", start=1000), rec("a_nss1", [(1102, 2498)], "GA", bc="CELL2", start=990),
          rec("a_nss2", [(1100, 2500)], "GA", bc="CELL3", start=1000)]
    R += [rec(f"a_x12_{i}", [(1600, 3001), (3100, 4500)], "GA", bc=f"CELL{i + 1}", start=1550) for i in range(2)]   # kinds 1, 2
    R += [rec(f"a_x21_{i}", [(1050, 1501), (1600, 3001)], "GA", bc=f"CELL{i + 1}", start=1000) for i in range(2)]   # kinds 2, 1
    R += [rec(f"a_inmodel{i}", [(1600, 2001), (2100, 3001)], "GA", start=1550) for i in range(2)]                   # inside TA3
    # GB: TB1's last read is on the other strand; a novel inside the evidenced TB1; a two-exon novel behind the two-exon TB2
    R += [rec("b1", TB1, "GB", "TB1", start=1000), rec("b_tb2", [(1100, 3001)], "GB", "TB2", start=1000), rec("b2", TB1, "GB", "TB1", start=1000, flag=16)]
    R += [rec(f"b_in{i}", [(2100, 3001), (3100, 4001)], "GB", start=2050) for i in range(2)]
    R += [rec(f"b_tie{i}", [(1100, 2700)], "GB", bc=f"CELL{i + 1}", start=1000) for i in range(2)]
    # GC1 / GC2: the chain 100, 102, 104 at DELTA 2 in two orders; GD: a record within DELTA of two founders
    ch = dict(a=[(100, 500)], b=[(102, 500)], c=[(104, 500)])
    R += [rec(f"c1{k}", ch[k], "GC1", start=50) for k in "abc"] + [rec("c1d", ch["c"], "GC1", start=50)]
    R += [rec(f"c2{k}", ch[k], "GC2", start=50) for k in order_gc2]
    R += [rec("d1", ch["a"], "GD", start=50), rec("d2", ch["c"], "GD", start=50), rec("d3", ch["b"], "GD", start=50), rec("d4", ch["c"], "GD", start=50)]
    # GE: a mono-exonic record and a founder of one record: the gene ends empty
    R += [rec("e_mono", [], "GE"), rec("e_one", ch["a"], "GE", start=50)]
    # GN (not in the refFlat): B is inside A, `sub` is inside A, C is inside B only (1104 is 4 from 1100)
    R += [rec(f"n_a{i}", TB1, "GN", start=1000) for i in range(2)]
    R += [rec(f"n_b{i}", [(1102, 2001), (2100, 3001)], "GN", start=1000) for i in range(2)]
    R += [rec(f"n_c{i}", [(1104, 2001)], "GN", start=1000) for i in range(2)]
    R += [rec(f"n_sub{i}", [(2100, 3001), (3100, 4001)], "GN", start=2050) for i in range(2)]
    # GO: evidence order is o2, o3, o4, o1 (chrB comes second in the dictionary): o1 joins o2's founder and is its last read
    R += [rec("o2", [(100, 500)], "GO", start=50), rec("o3", [(104, 500)], "GO", start=50), rec("o4", [(104, 500)], "GO", start=50)]
    return R


def hand_bam(**kw):
    return bammodel.bam_bytes(HEAD, REFS, hand_records(**kw))


# ---- generated cases -------------------------------------------------------------------------------------------------------------------
def _gene_ref(g, base, n_tx=2, n_exon=4):
    """n_tx lines of gene g: line k keeps exons 0 .. n_exon-1 but skips exon k + 1 when it can (shared splice sites)"""
    out = ""
    for k in range(n_tx):
        ex = [i for i in range(n_exon) if not (k > 0 and n_exon > 2 and i == 1 + (k - 1) % (n_exon - 2))]
        xs = [base + 1000 * i for i in ex]
        xe = [x + 100 for x in xs]
        out += (f"{g}\t{g}.T{k}\tchr12\t+\t{xs[0]}\t{xe[-1]}\t{xs[0]}\t{xe[-1]}\t{len(xs)}\t" + "".join(f"{x}," for x in xs) + "\t" +
                "".join(f"{x}," for x in xe) + "\n")
    return out


def sizes_case():
    """genes with 0, 1, 63, 64, 65 and BLOCK + 1 undef records (every record of a gene within DELTA of its first: one founder each)"""
    ref, R = "", []
    for gi, n in enumerate((0, 1, 63, 64, 65, BLOCK + 1)):
        g, base = f"S{n:03d}", 10000 + 20000 * gi
        ref += _gene_ref(g, base)
        R.append(rec(f"{g}_k", [(base + 100, base + 1001), (base + 1100, base + 2001), (base + 2100, base + 3001)], g, f"{g}.T0", start=base + 1))
        R += [rec(f"{g}_u{i}", [(base + 100 + i % 3, base + 2601)], g, bc=f"CELL{i % 5}", start=base + 1 - i % 7) for i in range(n)]
    return bammodel.bam_bytes(HEAD, REFS, R), ref, "".join(f"CELL{i}\n" for i in range(5))


def founders_case():
    """genes with 1, 63, 64, 65 and 300 founders: founder f of a gene has its donor at base + 100 + 5 f, and 1 + f % 3 records"""
    ref, R = "", []
    for gi, n in enumerate((1, 63, 64, 65, 300)):
        g, base = f"F{n:03d}", 10000 + 20000 * gi
        ref += _gene_ref(g, base)
        for k in range(3):                               # interleaved, so that a founder's records are spread over the list
            R += [rec(f"{g}_f{f}_{k}", [(base + 100 + 5 * f, base + 3001)], g, bc=f"CELL{(f + k) % 5}", start=base + 1) for f in range(n) if k <= f % 3]
    return bammodel.bam_bytes(HEAD, REFS, R), ref, "".join(f"CELL{i}\n" for i in range(5))


def junction_lists_case():
    """founders of 1, 63, 64, 65 and LDS_JUNC + 1 junctions, two records each (the second moved by DELTA), in one gene, apart from each other"""
    R = []
    for k, n in enumerate((1, 63, 64, 65, LDS_JUNC + 1)):
        j = [(10100 + 60000 * k + 40 * i, 10121 + 60000 * k + 40 * i) for i in range(n)]
        R += [rec(f"J{n}_0", j, "JL", start=j[0][0] - 99), rec(f"J{n}_1", [(a + 2, b - 2) for a, b in j], "JL", bc="CELL2", start=j[0][0] - 97)]
    return bammodel.bam_bytes(HEAD, REFS, R), _gene_ref("JL", 10000), "CELL1\nCELL2\n"


FILTER_TARGETS = (1, 63, 64, 65, 200)


def filter_lists_case():
    """genes whose first novel is tested against 1, 63, 64, 65 and 200 transcripts (a third of them kept with evidence, then the model's
    lines), the LAST of which contains it (dropped), and a second novel that none contains (kept)"""
    ref, R = "", []
    for gi, n in enumerate(FILTER_TARGETS):
        g, base = f"L{n:03d}", 10000 + 40000 * gi
        n_ev = n // 3
        mid = lambda k: base + (20000 if k == n - n_ev - 1 else 1000 + 10 * k)  # noqa: E731 -- the middle exon of line k
        for k in range(n - n_ev):
            ref += (f"{g}\t{g}.T{k}\tchr12\t+\t{base}\t{base + 30100}\t{base}\t{base + 30100}\t3\t{base},{mid(k)},{base + 30000},\t"
                    f"{base + 100},{mid(k) + 5},{base + 30100},\n")
        R += [rec(f"{g}_in{i}", [(base + 20005, base + 30001)], g, start=base + 20001) for i in range(2)]
        R += [rec(f"{g}_out{i}", [(base + 25000, base + 30001)], g, start=base + 24000) for i in range(2)]
        R += [rec(f"{g}_k{k}", [(base + 100, mid(k) + 1), (mid(k) + 5, base + 30001)], g, f"{g}.T{k}", start=base + 1) for k in range(n_ev)]
    return bammodel.bam_bytes(HEAD, REFS, R), ref, "CELL1\n"


def seeded_case(seed, n_genes=12, n_rec=1500):
    """records of n_genes six-exon genes of five lines: known evidence, and undef records over the genes' splice sites with jitter up to 3 (and
    now and then an acceptor inside an exon), RN 1 .. 3; the last gene is not in the refFlat"""
    rng = np.random.default_rng(seed)
    ref = "".join(_gene_ref(f"R{g:02d}", 10000 + 20000 * g, n_tx=5, n_exon=6) for g in range(n_genes))
    R = []
    for i in range(n_rec):
        gi = int(rng.integers(n_genes + 1))               # the last gene is not in the refFlat
        g, base = f"R{gi:02d}", 10000 + 20000 * gi
        jit = lambda: int(rng.integers(-1, 2)) * (3 if rng.random() < 0.1 else 1)  # noqa: E731
        kw = dict(bc=f"CELL{int(rng.integers(6))}", rn=int(rng.integers(1, 4)), flag=16 * int(rng.integers(2)), start=base + 1 - int(rng.integers(20)))
        if gi < n_genes and rng.random() < 0.2:
            ex = [0, 1, 2, 3, 4, 5]
            R.append(rec(f"r{i}", [(base + 1000 * a + 100, base + 1000 * b + 1) for a, b in zip(ex, ex[1:])], g, f"{g}.T0", **kw))
            continue
        ex = [0] + sorted(rng.choice(np.arange(1, 6), size=int(rng.integers(0, 5)), replace=False).tolist())
        junc = [(base + 1000 * a + 100 + jit(), base + 1000 * b + 1 + jit() + (40 if rng.random() < 0.1 else 0)) for a, b in zip(ex, ex[1:])]
        R.append(rec(f"r{i}", junc, g, **kw))
    return bammodel.bam_bytes(HEAD, REFS, R), ref, "".join(f"CELL{i}\n" for i in range(5))
