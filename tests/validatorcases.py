"""Inputs of the validator tests (test infrastructure only), built from literals and seeds on top of tests/collapsecases.py: the hand-built case
whose results tests/test_validator_cpu.py spells out, and the generators of the size, contention, table and order edges
tests/test_validator_gpu.py runs (each edge is asserted present with the model in test_validator_cpu.py)."""
import numpy as np

import bammodel
import collapsecases as cc

# SHORT's dictionary: another order than the ISOBAM's (chr12 is reference 1 here, 0 there), and no chrB
SHORT_HEAD = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrQ\tLN:2000000\n@SQ\tSN:chr12\tLN:2000000\n"
SHORT_REFS = [("chrQ", 2000000), ("chr12", 2000000)]
# with chrB: the keys chr12:100-500 and chrB:100-500 then differ in the reference id alone
SHORT_HEAD_B = "@HD\tVN:1.6\n@SQ\tSN:chrB\tLN:2000000\n@SQ\tSN:chrQ\tLN:2000000\n@SQ\tSN:chr12\tLN:2000000\n"
SHORT_REFS_B = [("chrB", 2000000), ("chrQ", 2000000), ("chr12", 2000000)]


def srec(name, pos1, cigar, ref_id=1, flag=0, mapq=60):
    """one record of SHORT: pos1 1-based, cigar [(op, length)]"""
    n = sum(ln for op, ln in cigar if op in "MIS=X")
    return bammodel.bam_record(name, flag, ref_id, pos1 - 1, mapq, cigar, "A" * n)


def spliced(donor, acceptor, left=51, right=30):
    """(pos1, cigar) of a record whose only boundary is (donor, acceptor)"""
    return donor - left + 1, [("M", left), ("N", acceptor - donor - 1), ("M", right)]


# ---- the hand-built case -----------------------------------------------------------------------------------------------------------------
def hand_records():
    """tests/collapsecases.py's records, and two genes more (neither in the refFlat): GP on the + strand of chrB, GQ with the junction
    (7100, 7101) that a zero-length N makes, which an insertion or a zero-length M in SHORT can support"""
    R = cc.hand_records()
    R += [cc.rec(f"p{i}", [(200, 600)], "GP", ref_id=1, start=150) for i in range(2)]
    R += [cc.rec(f"q{i}", [], "GQ", start=7001, cigar=[("M", 100), ("N", 0), ("M", 30)]) for i in range(2)]
    return R


def hand_bam():
    return bammodel.bam_bytes(cc.HEAD, cc.REFS, hand_records())


# CAGE: LF line ends, every text form.  The + starts on chr12 are 1000, 1500, 100, 4100; the one - end is 4151.
HAND_CAGE = ("track name=cage description=\"hand built\"\n"
             "browser position chr12:1-100\n"
             "# a comment\n"
             "\n"
             "chr12\t1000\t1010\tp1\t1.5\t+\n"                # exactly at txStart 1000
             "chr12 1500   1510 p2 0 +\n"                     # tokens separated by runs of spaces: 50 in front of txStart 1550
             "chr12\t100\t110\tp3\t0\t+\n"                    # 50 behind txStart 50
             "chr12\t50\t60\tp4\t0\t.\n"                      # strand '.': at txStart 50, never looked at
             "chr12\t50\n"                                    # two tokens: strand NONE
             "chr12\t50\t60\tp5\tx\t+\n"                      # a score Float.parseFloat refuses: strand NONE
             "chr12\t4000\t4151\tp6\t0\t-\n"                  # - strand: its END, 51 behind TB1's txEnd 4100
             "chr12\t4100\t4200\tp7\t0\t+\n"                  # the other strand exactly at TB1's txEnd
             "   \t \n")                                      # blank after trim
# POLYA: CRLF line ends.  Two ties at 7 in both file orders; chrB on the + strand only.
HAND_POLYA = ("chr12\t3037\t3040\ta\t0\t+\r\n"                # txEnd 3030: +7 here comes first: pos - pp = -7, dist +7
              "chr12\t3023\t3030\tb\t0\t+\r\n"
              "chr12\t2522\t2530\tc\t0\t+\r\n"                # txEnd 2529: -7 here comes first: pos - pp = 7, dist -7
              "chr12\t2536\t2540\td\t0\t+\r\n"
              "chr12\t5050\t5060\te\t0\t+\r\n"
              "chr12\t2729\t2740\tf\t0\t+\r\n"
              "chr12\t900\t1049\tg\t0\t-\r\n"                 # - strand: end 1049, 50 behind TB1's txStart 999
              "chrB\t600\t700\th\t0\t+\r\n")
# a BED line the parser fails on: {case: (line number, the line that stands there instead of HAND_CAGE's)}
BAD_BED_LINES = dict(
    start=(6, "chr12\t15o0\t1510\tp2\t0\t+"),
    end=(7, "chr12\t100\t\tp3\t0\t+"),
    blocks=(5, "chr12\t1000\t1010\tp1\t1.5\t+\t1000\t1010\t0\t2\t5,\t0,5"),           # two blocks, one size
    colour=(12, "chr12\t4100\t4200\tp7\t0\t+\t4100\t4200\t255,0"))


def bad_cage(which):
    no, bad = BAD_BED_LINES[which]
    lines = HAND_CAGE.split("\n")
    lines[no - 1] = bad
    return "\n".join(lines)


def hand_short_records(with_chr_b=False):
    """chr12 is reference 1 (2 with chrB in the dictionary)"""
    c12 = 2 if with_chr_b else 1
    s = lambda name, pos1, cigar, **kw: srec(name, pos1, cigar, **dict(dict(ref_id=c12), **kw))  # noqa: E731
    R = []
    # chr12:1100-5001, three records: N-made; D-made under clips with a pad in the gap; = / X blocks behind an insertion
    R += [s("j5001_n", 1050, [("M", 51), ("N", 3900), ("M", 30)])]
    R += [s("j5001_d", 1050, [("H", 5), ("S", 10), ("M", 51), ("D", 3900), ("P", 2), ("M", 30), ("S", 3)])]
    R += [s("j5001_eqx", 1050, [("=", 20), ("I", 1), ("X", 31), ("N", 3900), ("=", 30)])]
    R += [s("j5001_unmapped", 1050, [("M", 51), ("N", 3900), ("M", 30)], flag=4)]               # flag 0x4: supports nothing
    R += [s("j5001_chrQ", 1050, [("M", 51), ("N", 3900), ("M", 30)], ref_id=c12 - 1)]           # the same coordinates on chrQ
    R += [s("j5001_noref", 1050, [("M", 51), ("N", 3900), ("M", 30)], ref_id=-1)]
    # chr12:1100-2700, two records: a secondary one, a duplicate of mapq 0
    R += [s("j2700_sec", *spliced(1100, 2700), flag=0x100), s("j2700_dup", *spliced(1100, 2700), flag=0x400, mapq=0)]
    # chr12:1100-2500, one supplementary record, and a boundary off by one on either side of either end
    R += [s("j2500_sup", *spliced(1100, 2500), flag=0x800)]
    R += [s(f"j2500_off{k}", *spliced(1100 + a, 2500 + b)) for k, (a, b) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1)))]
    # chr12:1600-3001, four records (of Novel.5 and Novel.6 both); the last goes on over a junction nobody asks for.  3100-4500: none.
    R += [s(f"j3001_{i}", *spliced(1600, 3001)) for i in range(3)]
    R += [s("j3001_3", 1550, [("M", 51), ("N", 1400), ("M", 100), ("N", 98), ("M", 30)])]
    R += [s("j1501", *spliced(1050, 1501))]
    # chr12:100-500, two records (of GC1's Novel.10 and GD's Novel.13 both); 104-500: only boundaries off by one
    R += [s(f"j500_{i}", *spliced(100, 500)) for i in range(2)]
    R += [s(f"j500_off{k}", *spliced(104 + a, 500 + b)) for k, (a, b) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1)))]
    # GN's three junctions in one record
    R += [s("gn3", 1050, [("M", 51), ("N", 900), ("M", 100), ("N", 900), ("M", 100), ("N", 900), ("M", 30)])]
    # chr12:7100-7101: zero-length M repeat the boundary twice (counted once), and an insertion makes it
    R += [s("q_zero", 7001, [("M", 100), ("M", 0), ("M", 0), ("M", 30)]), s("q_ins", 7001, [("M", 100), ("I", 2), ("M", 30)])]
    # boundaries nobody asks for: a pad, = / X, a deletion; no CIGAR; one operation
    R += [s("pad", 3000, [("M", 10), ("P", 1), ("M", 10)]), s("eqx", 3000, [("=", 5), ("X", 1), ("=", 5)]), s("del", 3000, [("M", 10), ("D", 2), ("M", 10)])]
    R += [s("nocigar", 3000, []), s("oneop", 3000, [("M", 50)])]
    if with_chr_b:
        R += [s("b500", *spliced(100, 500), ref_id=0)]                                         # chrB:100-500, once
    return R


def hand_short(with_chr_b=False):
    return bammodel.bam_bytes(SHORT_HEAD_B if with_chr_b else SHORT_HEAD, SHORT_REFS_B if with_chr_b else SHORT_REFS, hand_short_records(with_chr_b))


# .txt columns 13-19 of the hand-built case at cageCo 50, polyaCo 50, juncCo 1, written out by hand:
# {(gene, transcript): (novelJunctions_reads, is_valid_allNovelJunctions, dist_cage, is_valid_cage, dist_polya, is_valid_polya, is_valid)}
MAXV = 2147483647
HAND_EXPECTED = {
    ("GA", "TA1"): (0, True, 1, True, -63, False, False),            # known: an empty list is true
    ("GA", "Novel.1"): (0, True, 0, True, 20, True, True),           # no novel junction: valid by CAGE and polyA alone
    ("GA", "Novel.5"): (4, False, -50, True, 521, False, False),     # 1600-3001: 4, 3100-4500: 0
    ("GA", "Novel.6"): (5, True, 0, True, 7, True, True),            # 1050-1501: 1, 1600-3001: 4 again
    ("GA", "Novel.2"): (3, True, 0, True, 20, True, True),
    ("GA", "Novel.4"): (1, True, 10, True, -7, True, True),
    ("GB", "TB1"): (0, True, -51, False, -50, True, False),          # its last read is on the - strand: ends, swapped positions
    ("GB", "TB2"): (0, True, 1, True, -63, False, False),
    ("GB", "Novel.9"): (2, True, 0, True, 0, True, True),
    ("GC1", "Novel.10"): (2, True, 50, True, 1993, False, False),
    ("GC1", "Novel.11"): (0, False, 50, True, 1993, False, False),
    ("GC2", "Novel.12"): (0, False, 50, True, 1993, False, False),
    ("GD", "Novel.13"): (2, True, 50, True, 1993, False, False),     # chr12:100-500 again: summed into both genes
    ("GD", "Novel.14"): (0, False, 50, True, 1993, False, False),
    ("GN", "Novel.16"): (3, True, 0, True, -993, False, False),
    ("GN", "Novel.18"): (0, False, 0, True, 492, False, False),
    ("GO", "Novel.20"): (0, False, MAXV, False, MAXV, False, False),   # chrB, - strand: in neither BED on that strand, not in SHORT
    ("GO", "Novel.21"): (0, False, 50, True, 1993, False, False),
    ("GP", "Novel.22"): (0, False, -MAXV, False, -29, True, False),    # chrB, + strand: not in CAGE
    ("GQ", "Novel.23"): (2, True, -2901, False, -2080, False, False),
}
# the valid novels per (cageCo, polyaCo, juncCo)
HAND_VALID = {(50, 50, 1): ["Novel.1", "Novel.6", "Novel.2", "Novel.4", "Novel.9"], (50, 50, 3): ["Novel.1", "Novel.2"],
              (0, 50, 1): ["Novel.1", "Novel.6", "Novel.2", "Novel.9"], (50, 0, 1): ["Novel.9"], (0, 0, 3): []}
HAND_SUPPORT = {("chr12", 1100, 5001): 3, ("chr12", 1100, 2700): 2, ("chr12", 1100, 2500): 1, ("chr12", 1600, 3001): 4, ("chr12", 3100, 4500): 0,
                ("chr12", 1050, 1501): 1, ("chr12", 100, 500): 2, ("chr12", 104, 500): 0, ("chr12", 102, 500): 0, ("chr12", 1100, 2001): 1,
                ("chr12", 2100, 3001): 1, ("chr12", 3100, 4001): 1, ("chr12", 1104, 2001): 0, ("chrB", 100, 500): 0, ("chrB", 200, 600): 0,
                ("chr12", 7100, 7101): 2}


# ---- generated cases ---------------------------------------------------------------------------------------------------------------------
FLAT_CAGE = "chr12\t0\t10\tc\t0\t+\nchr12\t0\t10\tc\t0\t-\n"
KEY_BASE = 10000


def keys_case(n_keys, per_key=2):
    """one gene (not in a refFlat) with n_keys two-exon novels, novel k with the junction (KEY_BASE + 100 k + 50, KEY_BASE + 100 k + 81):
    n_keys distinct keys -> (isobam, refflat, csv)"""
    R = []
    for k in range(n_keys):
        j = [(KEY_BASE + 100 * k + 50, KEY_BASE + 100 * k + 81)]
        R += [cc.rec(f"k{k}_{i}", j, "GK", bc=f"CELL{i + 1}", start=KEY_BASE + 100 * k + 1) for i in range(per_key)]
    return bammodel.bam_bytes(cc.HEAD, cc.REFS, R), "", "CELL1\nCELL2\n"


def key_junction(k):
    return KEY_BASE + 100 * k + 50, KEY_BASE + 100 * k + 81


def short_for_keys(n_keys, reads):
    """reads[k] records supporting key k, interleaved"""
    R = []
    for i in range(max(reads, default=0)):
        R += [srec(f"s{k}_{i}", *spliced(*key_junction(k)), ref_id=1) for k in range(n_keys) if i < reads[k]]
    return bammodel.bam_bytes(SHORT_HEAD, SHORT_REFS, R)


def short_sizes(n):
    """n records over the three keys of keys_case(3): record i supports key i % 3, every fourth is unspliced"""
    R = []
    for i in range(n):
        if i % 4 == 3:
            R.append(srec(f"u{i}", KEY_BASE + i, [("M", 100)]))
        else:
            R.append(srec(f"s{i}", *spliced(*key_junction(i % 3))))
    return bammodel.bam_bytes(SHORT_HEAD, SHORT_REFS, R)


LONG_OPS, LONG_BOUNDARIES = 300, 120
LONG_KEYS = (0, 63, 64, 119)     # the 1st, 64th, 65th and last boundary of the long CIGAR


def long_cigar_case():
    """a SHORT record of 300 operations and 120 boundaries: 121 M blocks and 120 N gaps, and 59 operations that make no boundary (clips at
    both ends, and in each of the first 55 gaps a pad or an insertion in front of the N), whose 1st, 64th, 65th and last boundary are the
    novel junctions of four two-exon novels -> (isobam, refflat, csv, short, the boundaries)"""
    pos1 = 50000
    cig, at, bounds = [("H", 3), ("S", 2)], pos1, []
    for b in range(LONG_BOUNDARIES + 1):
        cig.append(("M", 20))
        at += 20
        if b < LONG_BOUNDARIES:
            if b < 55:
                cig.append(("P", 1) if b % 2 == 0 else ("I", 2))
            cig.append(("N", 30 + b))
            bounds.append((at - 1, at + 30 + b))
            at += 30 + b
    cig += [("S", 4), ("H", 1)]
    assert len(cig) == LONG_OPS and len(bounds) == LONG_BOUNDARIES
    R = []
    for k in LONG_KEYS:
        R += [cc.rec(f"L{k}_{i}", [bounds[k]], "GL", bc=f"CELL{i + 1}", start=bounds[k][0] - 15) for i in range(2)]
    short = bammodel.bam_bytes(SHORT_HEAD, SHORT_REFS, [srec("long", pos1, cig), srec("plain", pos1, [("M", 100)])])
    return bammodel.bam_bytes(cc.HEAD, cc.REFS, R), "", "CELL1\nCELL2\n", short, bounds


def near_keys_case():
    """keys that differ in the reference id alone, in the donor alone, in the acceptor alone; one SHORT record for each but the last"""
    R = []
    for n, (ref_id, d, a) in enumerate(((0, 20050, 20081), (1, 20050, 20081), (0, 20051, 20081), (0, 20050, 20082))):
        R += [cc.rec(f"n{n}_{i}", [(d, a)], f"GN{n}", bc=f"CELL{i + 1}", ref_id=ref_id, start=20001) for i in range(2)]
    S = [srec("r0", *spliced(20050, 20081), ref_id=2), srec("r0b", *spliced(20050, 20081), ref_id=2), srec("r1", *spliced(20050, 20081), ref_id=0),
         srec("r2", *spliced(20051, 20081), ref_id=2)]
    return bammodel.bam_bytes(cc.HEAD, cc.REFS, R), "", "CELL1\nCELL2\n", bammodel.bam_bytes(SHORT_HEAD_B, SHORT_REFS_B, S)


def seeded_short(isobam, refflat, csv, seed, n_rec=20000, spliced_share=0.2):
    """n_rec 100-base records of SHORT for a collapse case on chr12: a fifth spliced, over the case's novel junctions: junction k of the
    sorted list is planted exactly (k % 3 == 0), off by one on one side (1) or left out for a junction nearby (2); records shuffled
    -> (short, spliced records per mode)"""
    import validatormodel as vm

    rng = np.random.default_rng(seed)
    order, genes, _cnt = vm.transcripts(isobam, refflat, csv)
    keys = sorted(set((d, a) for g in order for t in genes[g] if t.chrom == "chr12" for d, a in t.novel_junctions))
    R, modes = [], [0, 0, 0]
    n_spliced = int(n_rec * spliced_share) if keys else 0
    for i in range(n_rec):
        if i < n_spliced:
            k = int(rng.integers(len(keys)))
            d, a = keys[k]
            modes[k % 3] += 1
            if k % 3 == 2:
                d, a = d + 7, a + 9
            elif k % 3 == 1:
                d, a = (d + int(rng.choice((-1, 1))), a) if rng.random() < 0.5 else (d, a + int(rng.choice((-1, 1))))
            left = int(rng.integers(10, 91))
            R.append(srec(f"s{i}", d - left + 1, [("M", left), ("N", a - d - 1), ("M", 100 - left)], ref_id=1,
                          flag=int(rng.choice((0, 16, 0x100, 0x400))), mapq=int(rng.integers(0, 61))))
        else:
            R.append(srec(f"u{i}", int(rng.integers(10000, 300000)), [("M", 100)], ref_id=int(rng.integers(2)), flag=16 * int(rng.integers(2))))
    return bammodel.bam_bytes(SHORT_HEAD, SHORT_REFS, [R[i] for i in rng.permutation(len(R))]), modes
