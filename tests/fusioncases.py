"""Inputs of the FusionDetector tests (test infrastructure only), built from literals and seeds: the hand-built case whose outputs
tests/test_fusion_cpu.py spells out, and the generators of the size and key edges tests/test_fusion_gpu.py runs (each edge is asserted
present with the model in test_fusion_cpu.py)."""
import numpy as np

import bammodel
import tagbammodel as tm

HEAD = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr9\tLN:2000000\n@SQ\tSN:chr22\tLN:2000000\n"
REFS = [("chr9", 2000000), ("chr22", 2000000)]
M100 = [("M", 100)]


def rec(name, ge, bc="CELL1", umi="U", flag=0, mapq=60, rn=None, de=None, df=None, cigar=None, ref_id=0, pos0=999, extra=b""):
    aux = b""
    if bc is not None:
        aux += tm.aux_z("BC", bc)
    if umi is not None:
        aux += tm.aux_z("U8", umi)
    if ge is not None:
        aux += tm.aux_z("GE", ge)
    if rn is not None:
        aux += tm.aux_int("RN", "C", rn)
    if de is not None:
        aux += tm.aux_f("de", de)
    if df is not None:
        aux += tm.aux_f("df", df)
    return bammodel.bam_record(name, flag, ref_id, pos0, mapq, M100 if cigar is None else cigar, "ACGT", aux=aux + extra)


def bam(records):
    return bammodel.bam_bytes(HEAD, REFS, records)


# ---- the hand-built case ---------------------------------------------------------------------------------------------------------------
HAND_CSV = "CELL1-1\nCELL2\nCELL3\n"


def hand_records():
    R = []
    # the filter, reason by reason: none of these is kept
    R += [rec("f_nobc", "GA,GB", bc=None), rec("f_unmapped", "GA,GB", flag=4)]
    R += [rec("f_chim_start", "GA,GB", cigar=[("S", 10001)] + M100), rec("f_chim_end", "GA,GB", cigar=M100 + [("H", 10001)])]
    R += [rec("f_nogene", None), rec("f_emptygene", ""), rec("f_undefgene", "undef")]
    R += [rec("f_supp0", "GA,GB", flag=0x800, mapq=0), rec("f_sec0", "GA,GB", flag=0x100, mapq=0)]
    # kept at the edge: a clip of exactly MAXCLIP, a primary record of mapq 0
    R += [rec("k_clip", "GA", umi="UCLIP", cigar=[("S", 10000)] + M100 + [("H", 10000)]), rec("k_mapq0", "GA", umi="UP0", mapq=0, rn=1)]
    # a read of three records, the UMI on the middle one, a gene from each: BCR (bucket 0) comes before ABL1 (bucket 8)
    R += [rec("r3", "ABL1", umi=None), rec("r3", "BCR", umi="UMID", flag=0x800, ref_id=1), rec("r3", "ABL1", umi=None, flag=0x800)]
    # a read whose last record changes the barcode: CELL2:UB with GA and GB
    R += [rec("rbc", "GA", bc="CELL3", umi="UB"), rec("rbc", "GB", bc="CELL2", umi=None, flag=0x800)]
    # one, three, no genes; the split cases
    R += [rec("t3", "GA,GB,GC", umi="UT3"), rec("ca", ",A", umi="UC1"), rec("cb", "A,,B", umi="UC2"), rec("cc", "A,", umi="UC3"), rec("cd", ",", umi="UC4")]
    # two genes from one record, in both orders: different buckets (TMPRSS2 9, ERG 11) and a shared bucket (EML4, ALK: 0; Aa, BB: one hash)
    R += [rec("ab1", "ERG,TMPRSS2", umi="U2", df=0.25), rec("ab2", "TMPRSS2,ERG", umi="U3", bc="CELL2")]
    R += [rec("s1", "EML4,ALK", umi="US1"), rec("s2", "ALK,EML4", umi="US2", bc="CELL2"), rec("s3", "BB,Aa", umi="US3", bc="CELL3"),
          rec("s4", "Aa,BB", umi="US4", bc="CELL3")]
    # two genes from two reads, in both orders; pctId is that of the read added last, nbReads the number of reads
    R += [rec("x1", "BCR", bc="CELL3", umi="UX", de=0.1), rec("x2", "ABL1", bc="CELL3", umi="UX", de=0.2)]
    R += [rec("y1", "ABL1", bc="CELL3", umi="UY"), rec("y2", "BCR", bc="CELL3", umi="UY")]
    # not counted: no UMI (its key is CELL1:null); an unlisted cell.  Counted: the UMI whose text is null
    R += [rec("nu", "GA,GB", umi=None), rec("ul", "GA,GB", bc="CELLX", umi="UU"), rec("ln", "GA,GB", umi="null")]
    # "-1" against a list with it and without it; rn 7; de
    R += [rec("m1", "GA,GB", bc="CELL1-1", umi="UM1", rn=7), rec("m2", "GB,GA", bc="CELL2-1", umi="UM2", de=0.05, df=0.5)]
    # 10, 10 and 9 molecules: F1|F2 (buckets 11, 12) and F3|F4 (13, 14) are tied, F6|F5 (0, 15) stays unnamed
    R += [rec(f"p{i}", "F2,F1", bc=f"CELL{2 + i % 2}", umi=f"UA{i:02d}") for i in range(10)]
    R += [rec(f"q{i}", "F3,F4", bc="CELL3", umi=f"UB{i:02d}") for i in range(10)]
    R += [rec(f"w{i}", "F5,F6", bc="CELL2", umi=f"UC{i:02d}") for i in range(9)]
    return R


def hand_bam():
    return bam(hand_records())


# ---- generated cases -------------------------------------------------------------------------------------------------------------------
CSV5 = "".join(f"CELL{i}\n" for i in range(5))


def read_sizes_case():
    """reads of 1, 2, 63, 64 and 65 records, interleaved in the file; record k names GA or GB, the UMI is on the middle record only, the
    last record changes the barcode"""
    sizes = (1, 2, 63, 64, 65)
    R = []
    for k in range(max(sizes)):
        for n in sizes:
            if k < n:
                R.append(rec(f"read{n}", "GA" if k % 2 == 0 else "GB", bc="CELL1" if k == n - 1 else "CELL0", umi=f"U{n}" if k == n // 2 else None,
                             flag=0x800 if k else 0, rn=k % 3 + 1, de=0.01 * (k % 7)))
    return bam(R), CSV5


def molecule_sizes_case():
    """molecules of 1, 63, 64, 65 and 300 reads, interleaved; read k names GA or GB; de and rn differ between the first and the last read"""
    sizes = (1, 63, 64, 65, 300)
    R = []
    for k in range(max(sizes)):
        for n in sizes:
            if k < n:
                R.append(rec(f"mol{n}_r{k}", "GA" if k % 2 == 0 else "GB", bc=f"CELL{n % 5}", umi=f"UM{n}", de=0.001 * k, rn=1 if n != 64 else 1 + k % 2))
    return bam(R), CSV5


def gene_counts_case():
    """molecules of 1, 2, 3 and 65 distinct genes (the last over 13 reads of five fields each, every name twice)"""
    R = [rec("g1", "GA,GA", umi="UG1"), rec("g2", "GA,GB,GA", umi="UG2"), rec("g3", "GC,GA,GB", umi="UG3")]
    for k in range(13):
        R.append(rec(f"g65_r{k}", ",".join(f"N{5 * k + i:02d}" for i in range(5)), umi="UG65"))
        R.append(rec(f"g65_s{k}", ",".join(f"N{5 * k + 4 - i:02d}" for i in range(5)), umi="UG65"))
    return bam(R), CSV5


LONG = "L" * 200


def keys_case():
    """keys that are prefixes of one another and keys that differ in the last byte only, as read names, barcodes, UMIs and gene names;
    gene names of 1 and of 200 bytes; a ':' that moves between barcode and UMI (one molecule, as in the reference)"""
    R = []
    for i, nm in enumerate(("r", "ra", "rab", "rac", "ra")):                      # the second "ra" joins the first
        R.append(rec(nm, ("G", "GA", "GAB", "GAC", LONG)[i], umi="UK", bc="CELL0", flag=0x800 if i == 4 else 0))
    for i, u in enumerate(("U", "UA", "UAB", "UAC")):
        R += [rec(f"u{i}a", "G", umi=u, bc="CELL1"), rec(f"u{i}b", ("GA", "GAB", "GAC", "Z")[i], umi=u, bc="CELL1")]
    for i, b in enumerate(("CELL", "CELL2", "CELL22", "CELL23")):
        R += [rec(f"b{i}a", LONG, umi="UK", bc=b), rec(f"b{i}b", LONG[:-1] + "M", umi="UK", bc=b)]
    R += [rec("colon1", "GA", bc="CELL3:", umi="UQ"), rec("colon2", "GB", bc="CELL3", umi=":UQ")]
    return bam(R), CSV5 + "CELL22\nCELL3:\n"


def tight_table_case():
    """64 records = 64 reads = 64 gene fields in 32 molecules of two genes, 8 cells: with table_log2 = 6 every table is full"""
    R = [rec(f"t{i:02d}", f"T{i:02d}", bc=f"CELL{i % 16 // 2}", umi=f"UT{i // 2:02d}") for i in range(64)]
    return bam(R), "".join(f"CELL{i}\n" for i in range(8))


def none_counted_case():
    return bam([rec(f"n{i}", "GA", bc=f"CELL{i % 5}", umi=f"UN{i}") for i in range(70)]), CSV5


def rows_case(n_rows):
    """n_rows keys, key i with 1 + i % 3 molecules over the cells"""
    R = []
    for i in range(n_rows):
        R += [rec(f"k{i}_{j}", f"P{i:03d}A,P{i:03d}B", bc=f"CELL{(i + j) % 5}", umi=f"UR{i}_{j}") for j in range(1 + i % 3)]
    return bam(R), CSV5


def big_row_case():
    """a row with 1001 molecules in one cell and 3 in another"""
    R = [rec(f"big{i}", "BCR,ABL1", bc="CELL1" if i < 1001 else "CELL4", umi=f"UBIG{i}") for i in range(1004)]
    return bam(R), CSV5


def seeded_case(seed, n_rec=20000):
    """about n_rec records: a few thousand molecules of 1 .. 8 reads of 1 .. 3 records, about a tenth of them with two genes, some with
    three; 40 cells of which 32 are listed; now and then no UMI, a filtered record, RN, de or df"""
    rng = np.random.default_rng(seed)
    genes = [f"GENE{i}" for i in range(60)] + ["BCR", "ABL1", "EML4", "ALK", "TMPRSS2", "ERG"]
    R, i = [], 0
    while len(R) < n_rec:
        bc, umi = f"CELL{int(rng.integers(40)):02d}" + ("-1" if rng.random() < 0.3 else ""), f"UMI{int(rng.integers(200)):03d}"
        g0 = genes[int(rng.integers(len(genes)))]
        p = rng.random()
        pool = [g0] if p < 0.93 else [g0, genes[int(rng.integers(len(genes)))]] if p < 0.985 else [g0] + [genes[int(x)] for x in rng.integers(len(genes), size=2)]
        for _ in range(int(rng.integers(1, 9))):
            i += 1
            has_umi = rng.random() > 0.03
            for k in range(int(rng.choice([1, 1, 1, 2, 3]))):
                ge = ",".join(pool[int(x)] for x in rng.integers(len(pool), size=int(rng.integers(1, 3))))
                q = rng.random()
                kw = dict(mapq=0, flag=0x800) if q < 0.02 else dict(cigar=[("S", 20000)] + M100) if q < 0.04 else dict(flag=4) if q < 0.05 else {}
                if k and "flag" not in kw:
                    kw["flag"] = 0x800
                if q > 0.97:
                    ge = "undef"
                R.append(rec(f"read{i}", ge, bc=bc, umi=umi if has_umi and (k != 1 or rng.random() < 0.5) else None,
                             rn=int(rng.integers(1, 4)) if rng.random() < 0.3 else None, de=float(rng.integers(0, 200)) / 1000 if rng.random() < 0.7 else None,
                             df=0.5 if rng.random() < 0.2 else None, **kw))
    order = rng.permutation(len(R))                                              # the records of a read and the reads of a molecule apart
    return bam([R[int(x)] for x in order]), "".join(f"CELL{i:02d}\n" for i in range(32))
