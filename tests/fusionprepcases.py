"""Inputs of the ExportClippedReads / AddBamReadTags tests (test infrastructure only), built from literals and seeds: the hand-built cases
whose outputs tests/test_fusionprep_cpu.py spells out, and the generators of the size, key and table edges tests/test_fusionprep_gpu.py
runs (each edge is asserted present in test_fusionprep_cpu.py)."""
import numpy as np

import bammodel
import tagbammodel as tm

HEAD = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr9\tLN:2000000\n"
REFS = [("chr9", 2000000)]
M10 = [("M", 10)]
S200 = [("S", 200), ("M", 10)]


def rec(name, cigar, ge="G", bc="C", umi="U", us="ACGT", qs="IIII", extra=b"", flag=0):
    """a record with GE / BC / U8 / US / QS as Z attributes (None: left out) and `extra` behind them"""
    aux = b"".join(tm.aux_z(t, v) for t, v in (("GE", ge), ("BC", bc), ("U8", umi), ("US", us), ("QS", qs)) if v is not None)
    return bammodel.bam_record(name, flag, 0, 999, 60, cigar, "ACGT", aux=aux + extra)


def bam(records):
    return bammodel.bam_bytes(HEAD, REFS, records)


# ---- ExportClippedReads: the hand-built case (MINCLIP 150) ------------------------------------------------------------------------------
def hand_records():
    R = []
    # MINCLIP and MINCLIP + 1 at each end, S and H
    R += [rec("s150_x", [("S", 150)] + M10), rec("s151_x", [("S", 151)] + M10, us="AAAA", qs="!!!!")]
    R += [rec("e150", M10 + [("S", 150)]), rec("e151", M10 + [("S", 151)])]
    R += [rec("h150", [("H", 150)] + M10), rec("h151", [("H", 151)] + M10)]
    R += [rec("g150", M10 + [("H", 150)]), rec("g151", M10 + [("H", 151)])]
    # only the outermost operation counts; a CIGAR of one operation is first and last
    R += [rec("inner", [("H", 5), ("S", 200), ("M", 100)]), rec("one", [("S", 200)]), rec("one150", [("S", 150)])]
    # each of the three tags missing; US / QS missing, of unequal length, empty
    R += [rec("noge", S200, ge=None), rec("nobc", S200, bc=None), rec("noumi", S200, umi=None)]
    R += [rec("nous", S200, us=None), rec("noqs", S200, qs=None), rec("uneq", S200, us="ACGTACGT", qs="II"), rec("empty", S200, us="", qs="III")]
    # a leading '_', the empty name
    R += [rec("_lead_x", S200), rec("", S200, ge="GE2")]
    # the same key from two read names; the third one's US is no string, which nothing reads
    R += [rec("dup_a", S200, ge="GD", us="AC", qs="II"), rec("dup_b", S200, ge="GD", us="GT", qs="JJ"),
          rec("dup_c", S200, ge="GD", us=None, extra=tm.aux_h("US", "abcd"))]
    # a record that is not clipped reserves nothing (nor is its integer QS read)
    R += [rec("nc_1", M10, ge="GN", qs=None, extra=tm.aux_int("QS", "C", 7)), rec("nc_2", [("S", 300)] + M10, ge="GN", us="TTTT", qs="KKKK")]
    # the first clipped occurrence wins, with or without US
    R += [rec("fu_1", S200, ge="GF", us=None), rec("fu_2", S200, ge="GF", us="CCCC")]
    # '=': a leading clip in front of it, a trailing clip with an operation between
    R += [rec("eq", [("S", 200), ("=", 50)]), rec("eq2", [("=", 50), ("M", 10), ("S", 200)])]
    # a repeated tag keeps its last value; equal keys out of different fields
    R += [rec("rep", S200, bc="first", extra=tm.aux_z("BC", "last")), rec("a", S200, ge="b_c", bc="x"), rec("a_z", S200, ge="b", bc="c_x")]
    return R


def hand_bam():
    return bam(hand_records())


# records the reference's loop dies on: name -> (record, the same record in front of which nothing stops)
STOPS = dict(
    underscores=lambda: rec("___", M10),
    a_typed_bc=lambda: rec("abc", M10, bc=None, extra=tm.aux_a("BC", "x")),
    h_typed_us=lambda: rec("hus", S200, ge="GH", us=None, extra=tm.aux_h("US", "abcd")),
    int_typed_qs=lambda: rec("iqs", S200, ge="GI", qs=None, extra=tm.aux_int("QS", "C", 3)),
    no_cigar=lambda: rec("nocigar", []),
    eq_clip=lambda: rec("eqclip", [("M", 10), ("=", 50), ("S", 30)]),
    eq_clip_2=lambda: rec("eqclip2", [("S", 200), ("=", 50), ("H", 1)]),
)


def stop_bam(which, at=20):
    R = hand_records()
    return bam(R[:at] + [STOPS[which]()] + R[at:])


# ---- AddBamReadTags: the hand-built case ------------------------------------------------------------------------------------------------
READ_NAMES = ["a_b", "g_c_u", "x_g_c_u", "a_b_c_d_e", "a_b_c_", "a_b__", "_a_b", "a__b_c", "___", "", "GENE1_CELLACGT_UMI12345", "r1_GENE1_CELL_UMI",
              "null_null_null"]


def read_records():
    aux = [b"", tm.aux_z("GE", "old") + tm.aux_int("BC", "C", 5) + tm.aux_z("U8", "old") + tm.aux_int("NM", "C", 2), tm.aux_z("AA", "x") + tm.aux_z("ZZ", "y")]
    return [bammodel.bam_record(nm, 4 if k % 4 == 3 else 0, -1 if k % 4 == 3 else 0, 100 + k, 60, [] if k % 4 == 3 else M10, "ACGT", aux=aux[k % 3])
            for k, nm in enumerate(READ_NAMES)]


def read_bam():
    return bam(read_records())


# ---- generated cases ----------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 70000]


def lengths_case():
    """every US / QS length of LENGTHS with the sequence's first byte at each of the four alignments of the output (the name is padded to
    steer it), QS one list entry further than US"""
    rng = np.random.default_rng(21)
    R, o = [], 0
    for j, L in enumerate(LENGTHS):
        Q = LENGTHS[(j + 1) % len(LENGTHS)]
        for target in range(4):
            base = f"L{L}t{target}"
            klen = len(base) + len("_G_C_U")
            pad = (target - (o + 1 + klen + 1)) % 4
            name = base + "p" * pad
            us = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, L))
            qs = "".join(chr(33 + int(x)) for x in rng.integers(0, 60, Q))
            R.append(rec(name, S200, us=us, qs=qs))
            o += 1 + klen + pad + 1 + L + 3 + Q + 1
    return bam(R)


DUP_SIZES = [1, 2, 63, 64, 65]


def dup_case():
    """one key 1 / 2 / 63 / 64 / 65 times, the groups interleaved so that each spreads over the file; every record has its own US"""
    groups = [[rec(f"d{k}_{j}", S200, ge=f"G{k}", us="ACGT" * (1 + j % 3) + f"N{j}", qs="I") for j in range(k)] for k in DUP_SIZES]
    R = []
    for j in range(max(DUP_SIZES)):
        R += [g[j] for g in groups if j < len(g)]
    return bam(R)


def prefix_case():
    """keys that are prefixes of one another, keys that differ in the last byte only, equal keys out of different fields"""
    R = [rec(nm, S200, umi=u) for nm in ("ab", "abc", "abcd", "a") for u in ("AAAA", "AAAB", "AAA", "AAAAA")]
    R += [rec("p", S200, ge="", bc="", umi=""), rec("p", S200, ge="", bc="", umi="_"), rec("p_", S200, ge="", bc="_", umi=""), rec("p", S200, ge="_", bc="", umi="")]
    return bam(R + R[::-1])


def fnv1a(b):
    h = 14695981039346656037
    for c in b:
        h = ((h ^ c) * 1099511628211) & (2 ** 64 - 1)
    return h


def slot(key, slots):
    """K-CLIP-INSERT's home slot of a key in a table of `slots`"""
    h = fnv1a(key)
    return (h ^ (h >> 32)) & (slots - 1)


def last_slot_umis(n, slots=512):
    """n UMIs whose key w_G_C_<umi> has the last slot of a table of `slots` (and of every smaller one) as its home"""
    out, u = [], 0
    while len(out) < n:
        if slot(f"w_G_C_{u:07d}".encode(), slots) == slots - 1:
            out.append(f"{u:07d}")
        u += 1
    return out


def distinct_case(n, wrap=0, dups=True):
    """n distinct keys, `wrap` of them sharing the table's last slot as their home; with dups every other key a second time (it loses)"""
    umis = last_slot_umis(wrap) if wrap else []
    R = [rec(f"w_{j}", S200, umi=umis[j]) if j < wrap else rec(f"k{j}_x", S200, umi=f"U{j * 7919 % 1000:03d}", us="AC" * (j % 5), qs="I" * (j % 7)) for j in range(n)]
    return bam(R + [rec(f"k{j}_y", S200, umi=f"U{j * 7919 % 1000:03d}", us="late") for j in range(wrap, n if dups else 0)])


def none_clipped_case():
    return bam([rec(f"n{j}_x", [("S", 150), ("M", 10), ("H", 150)], umi=f"U{j}") for j in range(100)])


def seeded_case(seed, n=20000):
    """about n records, shuffled: a third clipped, some 2500 keys with duplicates among and across them, all five attributes now and then
    missing, names with and without '_'"""
    rng = np.random.default_rng(seed)
    R = []
    for j in range(n):
        k = int(rng.integers(2500))
        clip = int(rng.integers(3)) == 0
        n_clip = int(rng.integers(151, 400)) if clip else int(rng.integers(0, 151))
        cigar = [[("S", n_clip)] + M10, M10 + [("H", n_clip)], [("S", n_clip), ("M", 30), ("S", 3)]][int(rng.integers(3))] if n_clip else M10
        L = int(rng.integers(0, 300))
        us = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, L)) if rng.integers(40) else None
        qs = "I" * L if rng.integers(40) else None
        name = f"read{k % 50}" + ("_" + str(j) if rng.integers(4) else "")
        R.append(rec(name, cigar, ge=f"GENE{k % 40}" if rng.integers(30) else None, bc=f"CELL{k % 25:02d}ACGTACGTAC", umi=f"UMI{k:06d}" if rng.integers(30) else None,
                     us=us, qs=qs))
    return bam(R)


# ---- step 6 as a chain ------------------------------------------------------------------------------------------------------------------
CHAIN_CSV = "CELL1\nCELL2\nCELL3\n"


def chain_records():
    """long reads with clips: two genes meet in the molecules of the same (cell, UMI); the read names end in _<n> as scanfastq writes them"""
    R = []
    for j in range(60):
        cell, umi = f"CELL{1 + (j // 2) % 3}", f"UMI{j // 2:04d}"
        ge = ("BCR", "ABL1")[j % 2] if j < 40 else "GAPDH"
        cigar = [("S", 151 + j)] + M10 if j % 5 else [("S", 20)] + M10
        R.append(rec(f"r{j:03d}_{j % 4}", cigar, ge=ge, bc=cell, umi=umi, us="ACGT" * (40 + j), qs="I" * (160 + 4 * j)))
    return R


def remapped_bam(fastq):
    """what minimap2 + samtools would hand on: one mapped record per FASTQ record, named like it, no attribute but NM and de"""
    names = [ln[1:].decode() for ln in fastq.split(b"\n")[0::4] if ln]
    recs = [bammodel.bam_record(nm, 0, 0, 1000 + 10 * k, 60, [("M", 100)], "ACGT", aux=tm.aux_int("NM", "C", 1) + tm.aux_f("de", 0.01)) for k, nm in enumerate(names)]
    return bam(recs)


def damaged_cases():
    """name -> a BAM with one clipped record whose attributes no walker accepts (tests/auxcases.py DAMAGED) between good ones, for
    K-CLIP-FLAG's clean refusal"""
    import auxcases
    return {k: bam(hand_records()[:4] + [rec("damaged", S200, extra=v)] + hand_records()[4:8]) for k, v in auxcases.DAMAGED.items()}
