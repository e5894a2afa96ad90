"""Input builders of tests/test_matrix_edges_cpu.py and tests/test_matrix_edges_gpu.py (test infrastructure only): BAMs, SNP files, cell
lists and refFlats that put K-MTX, K-SNP and K-ISO on the edges of their loops -- the 64-lane batches, the carried sums between CIGAR
rounds, the digit widths of the renderer, the LDS / HBM boundary of the candidate counts.  Everything is generated from fixed seeds, and
every builder also returns what its construction makes the answer, so that a mistake shared by the Python model and a kernel still fails."""
import functools

import numpy as np

import bammodel
import isoformmodel as im
import snpmodel as sm
import tagbammodel as tm

SNP_LN = 1 << 29
SNP_HEAD = f"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:{SNP_LN}\n@SQ\tSN:chr2\tLN:1000000\n@SQ\tSN:chr3\tLN:1000000\n"
SNP_REFS = [("chr1", SNP_LN), ("chr2", 1000000), ("chr3", 1000000)]
MOLHEAD = "cellBC\tUMI\tnbReads\tnbSupportingReads\tmappingPctId\tsnpPhredScore\tgeneId\ttranscriptId\n"
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def srec(name, cigar, pos1, bc, umi, rn=b"", flag=0, ref=0, seq=None, qual=None, pre=b""):
    """a record of the SNP cases; rn: the RN attribute's bytes; pre: attribute bytes in front of BC / U8 / RN"""
    n = sum(ln for op, ln in cigar if op in "MIS=X")
    seq = sm.seq_of(n) if seq is None else seq
    aux = pre + (tm.aux_z("BC", bc) if bc is not None else b"") + (tm.aux_z("U8", umi) if umi is not None else b"") + rn
    return bammodel.bam_record(name, flag, ref, pos1 - 1, 60, cigar, seq, sm.qual_of(len(seq)) if qual is None else qual, aux=aux)


def snp_bam(recs):
    return bammodel.bam_bytes(SNP_HEAD, SNP_REFS, recs)


@functools.lru_cache(maxsize=None)
def snp_model(case, csv=None, min_rn=0, min_qv=0):
    """the model's answer of a named SNP case (computed once per process, shared by every test that needs it)"""
    c = SNP_CASES[case]()
    return sm.snp_matrix(c["bam"], c["snp"], c["csv"] if csv is None else csv, min_rn=min_rn, min_qv=min_qv)


# ---- (a) the renderer: counts per (row, cell) known by construction ---------------------------------------------------------------------
COUNTS = (0, 1, 9, 10, 11, 99, 100, 101, 999, 1000, 1001)
N_HIT_CELLS = 200
RENDER_ROWS = 5


def render_counts():
    """{(row, hit cell): distinct UMIs}: every value of COUNTS side by side across the 64-cell boundary (row 0), again at the start of row
    1 with more of them on both sides of cells 63 | 64 and 127 | 128, a row whose only hit is in the last hit cell (C199: the row exists
    only where that cell is listed, render_cell_names(201) or zz=False), and two sparse rows"""
    n = {}
    for i, c in enumerate(COUNTS):
        n[(0, 58 + i)] = c
    for i, c in enumerate(reversed(COUNTS)):
        n[(1, i)] = c
    n.update({(1, 63): 1001, (1, 64): 9, (1, 65): 100, (1, 127): 10, (1, 128): 999, (1, 198): 100, (2, 199): 11,
              (3, 0): 1, (3, 62): 99, (3, 63): 10, (3, 64): 11, (3, 129): 101, (4, 0): 10, (4, 127): 1})
    return {k: v for k, v in n.items() if v}


def render_cell_names(n_listed, zz=True):
    """(the listed names, sorted).  One name: the first hit cell.  More: the first n - 1 hit cells and ZZ, a listed cell without a hit in
    the last column; the hit cells behind them are hit but not listed (201 lists every hit cell).  zz=False: the first n hit cells and
    no ZZ, so that the last column, directly in front of the line feed, holds counts."""
    hit = [f"C{k:03d}" for k in range(N_HIT_CELLS)]
    return hit[:n_listed] if n_listed == 1 or not zz else hit[:n_listed - 1] + ["ZZ"]


def _umi_records(rng, counts, pos_of, name_of, multi_below=None):
    """records 2M at pos_of(row) of cell name_of(cell), n distinct UMIs per (row, cell), 1 to 3 records per UMI (only UMIs below
    multi_below, where given); the repeats are shuffled into the tail of the file, far from their first record"""
    first, tail = [], []
    for (r, k), n in sorted(counts.items()):
        reps = rng.integers(1, 4, n)
        for j in range(n):
            bc = name_of(k) + ("-1" if (k + j) % 2 else "")
            for t in range(int(reps[j]) if multi_below is None or j < multi_below else 1):
                (tail if t else first).append(srec(f"r{r}_{k}_{j}_{t}", [("M", 2)], pos_of(r), bc, f"U{j:06d}", seq="AC", qual=b"\x1e\x1f"))
    return [first[i] for i in rng.permutation(len(first))] + [tail[i] for i in rng.permutation(len(tail))], len(first), len(tail)


def render_gene(r):
    """row 0's name is longer than the others', so that its row books more bytes and a block can end behind it alone"""
    return f"g{r}" + "x" * 40 * (r == 0)


def _render_text(counts, names, n_rows, pos_of):
    """(matrix text, metrics text, row labels) the construction gives for the listed names (byte order)"""
    names = sorted(names)
    mat = ["geneId\ttranscriptId\tnbExons" + "".join("\t" + c for c in names) + "\n"]
    met = ["geneId\ttranscriptId\tnbExons\tnbUmis\n"]
    labels = []
    for r in range(n_rows):
        vals = [counts.get((r, c), 0) for c in names]
        if any(vals):
            label = f"{render_gene(r)}\tchr1:{pos_of(r)}..A\tna"
            labels.append(label)
            mat.append(label + "".join(f"\t{v}" for v in vals) + "\n")
            met.append(f"{label}\t{sum(vals)}\n")
    return "".join(mat).encode(), "".join(met).encode(), labels


def _render_pos(r):
    return 1000 + 10 * r


@functools.lru_cache(maxsize=None)
def render_case():
    rng = np.random.default_rng(101)
    counts = render_counts()
    recs, n_first, n_tail = _umi_records(rng, counts, _render_pos, lambda k: f"C{k:03d}")
    snp = "".join(f"chr1,{_render_pos(r)},+,{render_gene(r)}\n" for r in range(RENDER_ROWS))
    return dict(bam=snp_bam(recs), snp=snp, csv=render_csv(N_HIT_CELLS), counts=counts, n_first=n_first, n_tail=n_tail)


def render_csv(n_listed, zz=True):
    return "".join(c + "\n" for c in render_cell_names(n_listed, zz))


def render_expected(n_listed, zz=True):
    names = render_cell_names(n_listed, zz)
    by_name = {(r, f"C{k:03d}"): v for (r, k), v in render_counts().items()}
    return _render_text(by_name, names, RENDER_ROWS, _render_pos)


WIDE_CELLS = ("A", "B", "C")
WIDE_COUNTS = {(0, 0): 7, (0, 1): 10001, (0, 2): 345, (1, 0): 100003, (1, 2): 10, (2, 0): 1000, (2, 1): 99, (2, 2): 9}


@functools.lru_cache(maxsize=None)
def wide_case():
    """three rows, three cells, every field width from 1 to 6 digits; 100,003 distinct UMIs in the middle row.  The first 1,500 UMIs of
    every (row, cell) have 1 to 3 records, the others one, so that the case stays a few seconds long."""
    rng = np.random.default_rng(102)
    recs, n_first, n_tail = _umi_records(rng, WIDE_COUNTS, _render_pos, lambda k: WIDE_CELLS[k], multi_below=1500)
    snp = "".join(f"chr1,{_render_pos(r)},+,{render_gene(r)}\n" for r in range(3))
    return dict(bam=snp_bam(recs), snp=snp, csv="".join(c + "\n" for c in WIDE_CELLS), n_first=n_first, n_tail=n_tail)


def wide_expected():
    return _render_text({(r, WIDE_CELLS[k]): v for (r, k), v in WIDE_COUNTS.items()}, WIDE_CELLS, 3, _render_pos)


def render_row_bytes(n_cells, label, widest):
    """the device bytes smi_mtx.h's matrix() books for one row of a block: dense counts, the label, the widest field per cell, the line
    feed, the row's length"""
    return n_cells * 4 + len(label) + n_cells * (1 + len(str(widest))) + 1 + 8


def render_blocks(labels, n_cells, widest, budget):
    """the row blocks matrix() makes under `budget`: rows while they fit, at least one"""
    blocks, cur, used = [], [], 0
    for r, label in enumerate(labels):
        rb = render_row_bytes(n_cells, label, widest)
        if cur and used + rb > budget:
            blocks.append(cur)
            cur, used = [], 0
        cur.append(r)
        used += rb
    return blocks + [cur]


def render_budgets():
    """{name: (budget_bytes, the row blocks it gives)} for the five rows of render_expected(201); row 1 holds the widest count, row 0
    books 40 bytes more than the others"""
    labels = render_expected(201)[2]
    rb = [render_row_bytes(201, lab, 1001) for lab in labels]
    return dict(around=(rb[1], [[0], [1], [2], [3], [4]]),                          # breaks directly in front of row 1 and behind it
                before_only=(rb[1] + rb[2], [[0], [1, 2], [3, 4]]),
                after_only=(rb[0] + rb[1], [[0, 1], [2, 3], [4]]),
                none=(rb[0] + rb[1] + rb[2], [[0, 1, 2], [3, 4]]),
                less_than_a_row=(10, [[0], [1], [2], [3], [4]]))


# ---- (b) K-SNP candidate search --------------------------------------------------------------------------------------------------------
OVERLAPS = (0, 1, 63, 64, 65, 128, 200)


def _acgt(rng, n):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n))


@functools.lru_cache(maxsize=None)
def search_case(bad_rn=False):
    """-> dict(bam, snp, csv, hits: per line of the file, rows).  bad_rn: the record that only the wide line reaches carries an RN of type
    Z, which the reference cannot cast: the run then has to stop naming that read, which shows the record was looked at."""
    rng = np.random.default_rng(202)
    recs, lines, rows = [], [], []

    def add(chrom, pos, strand, name, hits, base=None):
        text = "|".join(map(str, pos))
        lines.append((f"{chrom},{text},{strand},{name}", hits))
        if hits:
            rows.append(f"{name}\t{chrom}:{text}..{base}\tna")

    for idx, n in enumerate(OVERLAPS):                       # one record under n lines of its strand, as many of the other strand between
        s = 100000 * (idx + 1)                               # them, and as many that end one base in front of it
        seq = _acgt(rng, 300)
        recs.append(srec(f"ov{n}", [("M", 300)], s, f"OV{n}", "U", seq=seq))
        for i in range(max(n, 1)):
            add("chr1", [s - 1], "+", f"o{n}before{i}", 0)
            add("chr1", [s + 1 + i], "-", f"o{n}rev{i}", 0)
            if n:
                add("chr1", [s + 1 + i], "+", f"o{n}hit{i}", 1, seq[1 + i])
    s = 900000                                               # inclusive borders: 100M5S covers s .. s + 99
    seq = _acgt(rng, 105)
    recs.append(srec("border", [("M", 100), ("S", 5)], s, "BORDER", "U", seq=seq))
    add("chr1", [s - 1], "+", "b_before", 0)
    add("chr1", [s], "+", "b_start", 1, seq[0])
    add("chr1", [s + 99], "+", "b_end", 1, seq[99])
    add("chr1", [s + 100], "+", "b_behind", 0)
    # the running maximum: `wide` starts in front of 400 short lines and ends far behind them
    s = 2000000
    seq = _acgt(rng, 105)
    recs.append(srec("spliced", [("M", 50), ("N", 400000), ("M", 50), ("S", 5)], s, "SPLICED", "U", seq=seq))
    add("chr1", [s + 400060, s + 10], "+", "wide", 1, seq[10] + seq[60])
    seq = _acgt(rng, 4100)
    recs.append(srec("short_only", [("M", 4100)], s + 100, "SHORT", "U", seq=seq))          # in spliced's intron, under the short lines
    for i in range(400):
        add("chr1", [s + 100 + 10 * i], "+", f"short{i}", 1, seq[10 * i])
    recs.append(srec("wide_only", [("M", 100), ("S", 5)], s + 100000, "WIDEONLY", "U",       # behind every short line, inside `wide`
                     rn=tm.aux_z("RN", "5") if bad_rn else b""))
    s = 3000000                                              # several lines of one first position
    seq = _acgt(rng, 105)
    recs.append(srec("same_first", [("M", 100), ("S", 5)], s, "SAME", "U", seq=seq))
    add("chr1", [s + 10], "+", "f_one", 1, seq[10])
    add("chr1", [s + 10, s + 13], "+", "f_two", 1, seq[10] + seq[13])
    add("chr1", [s + 12, s + 10, s + 11], "+", "f_three", 1, seq[10:13])
    add("chr1", [s + 10, s + 200], "+", "f_out", 0)
    add("chr1", [s + 10], "-", "f_rev", 0)
    recs.append(srec("on_chr2", [("M", 100), ("S", 5)], 5000, "CHR2", "U", ref=1))          # a reference without lines
    add("chr3", [5010], "+", "chr3_line", 0)                                                 # a reference without records
    recs.append(bammodel.bam_record("unmapped", 4, -1, -1, 0, [], "ACGT", b"\x1e" * 4, aux=tm.aux_z("BC", "UNMAPPED") + tm.aux_z("U8", "U")))
    order = rng.permutation(len(lines))
    lines = [lines[i] for i in order]
    cells = [f"OV{n}" for n in OVERLAPS] + ["BORDER", "SPLICED", "SHORT", "WIDEONLY", "SAME", "CHR2", "UNMAPPED"]
    return dict(bam=snp_bam([recs[i] for i in rng.permutation(len(recs))]), snp="".join(t + "\n" for t, _h in lines),
                csv="".join(c + "\n" for c in cells), hits=[(t, h) for t, h in lines], rows=sorted(rows, key=str.encode))


N_TABLE_CELLS = 8191      # smi_snp_create: the smallest power of two >= 2 * cells + 2 = 16384 slots, load factor 0.49994 -- the fullest
#                           table the host ever builds (one cell more doubles the table)


def table_names():
    """N0 .. N8189 (N1 is a prefix of N10, N100, ...) and the empty name, which is what the barcode "-1" becomes"""
    return [f"N{i}" for i in range(N_TABLE_CELLS - 1)] + [""]


def table_barcode(i, name):
    """the barcode as the BAM writes it: "-1" nowhere, at the end, in the middle, twice, in front"""
    if name == "":
        return "-1"
    return (name, name + "-1", name[:1] + "-1" + name[1:], name[:2] + "-1" + name[2:] + "-1", "-1" + name)[i % 5]


@functools.lru_cache(maxsize=None)
def table_case():
    rng = np.random.default_rng(203)
    names = table_names()
    recs = [srec(f"t{i}", [("M", 2)], 7000, table_barcode(i, nm), f"U{i}", seq="GA", qual=b"\x14\x15") for i, nm in enumerate(names)]
    recs += [srec(f"x{i}", [("M", 2)], 7000, bc, "UX", seq="GA", qual=b"\x14\x15") for i, bc in enumerate(("N", "N8190", "N12x", "-", "1", "N-"))]
    csv = "".join(("-1" if nm == "" else nm + "-1" if i % 3 == 0 else nm) + "\n" for i, nm in enumerate(names))
    return dict(bam=snp_bam([recs[i] for i in rng.permutation(len(recs))]), snp="chr1,7000,+,site\n", csv=csv, n_unlisted=6)


def table_expected():
    names = sorted(table_names(), key=str.encode)
    return ("geneId\ttranscriptId\tnbExons" + "".join("\t" + c for c in names) + "\n" + "site\tchr1:7000..G\tna" + "\t1" * len(names) + "\n").encode()


# ---- (c) K-SNP CIGAR walk --------------------------------------------------------------------------------------------------------------
GAPS = "IDNP"
WALK_OPS = (1, 63, 64, 65, 127, 128, 129, 300)


def gen_cigar(rng, n_ops, forced=None, lengths=None):
    """exactly n_ops operations of M = X I D N S H P from the seeded generator: H, S only at the ends, a gap (I D N P) always between two
    of M = X, no operation twice in a row; forced: {index: op}, lengths: {index: length}.  Only CIGARs the reference's junction walk
    (isoformmodel.junctions) accepts are returned."""
    forced, lengths = forced or {}, lengths or {}
    while True:
        lead = [[], ["S"], ["H"], ["H", "S"]][int(rng.integers(4))] if n_ops >= 9 and min(forced, default=99) > 2 else []
        trail = [[], ["S"], ["H"], ["S", "H"]][int(rng.integers(4))] if n_ops >= 9 and max(forced, default=0) < n_ops - 3 else []
        ops = list(lead)
        end = n_ops - len(trail)
        while len(ops) < end:
            i = len(ops)
            prev = ops[-1] if ops else "H"
            if i in forced:
                op = forced[i]
            elif prev not in "M=X" or i == end - 1 or forced.get(i + 1, "M") in GAPS or rng.random() < 0.55:
                op = "M=X".replace(prev, "")[int(rng.integers(2 if prev in "M=X" else 3))]
            else:
                op = GAPS[int(rng.integers(4))]
            ops.append(op)
        ops += trail
        ok = all(a != b for a, b in zip(ops, ops[1:])) and ops[len(lead)] in "M=X" and ops[end - 1] in "M=X"
        ok = ok and all(ops[i - 1] in "M=X" and ops[i + 1] in "M=X" for i in range(len(lead), end) if ops[i] in GAPS)
        if not ok:
            continue
        size = {"M": (2, 7), "=": (2, 7), "X": (1, 4), "I": (1, 4), "D": (1, 26), "N": (30, 200), "P": (1, 3), "S": (1, 9), "H": (1, 9)}
        cig = [(op, lengths.get(i, int(rng.integers(*size[op])))) for i, op in enumerate(ops)]
        try:
            im.junctions(1000, cig)
        except im.IsoformError:
            continue
        return cig


def cigar_table(pos1, cigar):
    """per operation (op, length, reference start, 1-based read offset of its first base) -- cumulative sums, not the model's walk"""
    ln = np.array([n for _op, n in cigar], dtype=np.int64)
    on_ref = np.array([op in "M=XDN" for op, _n in cigar])
    on_read = np.array([op in "M=XIS" for op, _n in cigar])
    ref = pos1 + np.concatenate([[0], np.cumsum(ln * on_ref)[:-1]])
    read = 1 + np.concatenate([[0], np.cumsum(ln * on_read)[:-1]])
    return [(op, int(n), int(ref[i]), int(read[i])) for i, (op, n) in enumerate(cigar)]


@functools.lru_cache(maxsize=None)
def walk_case():
    """-> dict(bam, snp, csv, lines): per line of the file dict(text, gene, pos_text, ok, bases, quals, rn, bc, umi, ops): ok: the
    construction says the line resolves on its one record; ops: the (0-based) operations its positions lie on"""
    rng = np.random.default_rng(303)
    recs, lines, cells = [], [], []

    def add(tag, pos, rec_info, ops=(), force_fail=False):
        """one line of positions `pos` (any order) against the record described by rec_info"""
        tab, seq, qual, neg, bc, umi, rn = rec_info
        rp = []
        for p in sorted(pos):
            hit = [q + p - r for op, n, r, q in tab if op in "M=X" and r <= p < r + n]
            rp.append(hit[0] if hit and hit[0] < len(seq) else 0)
        ok = all(rp) and not force_fail
        bases = "".join((COMPLEMENT.get(seq[x - 1], "") if neg else seq[x - 1]) for x in rp) if ok else None
        text = "|".join(map(str, pos))
        lines.append(dict(text=f"chr1,{text},{'-' if neg else '+'},{tag}", gene=tag, pos_text=text, ok=ok, bases=bases,
                          quals=[qual[x - 1] for x in rp] if ok else None, rn=rn, bc=bc, umi=umi, ops=tuple(ops)))

    def record(name, cig, start, neg=False, seq=None, qual=None, rn=b"", rn_value=1, pre=b"", bc=None):
        n = sum(ln for op, ln in cig if op in "MIS=X")
        seq = "".join("ACGTN"[int(x)] for x in rng.choice(5, n, p=[0.24, 0.24, 0.24, 0.24, 0.04])) if seq is None else seq
        qual = bytes([7] + [int(x) for x in rng.integers(0, 120, n - 1)]) if qual is None else qual
        bc = bc or name.upper()
        cells.append(bc)
        recs.append(srec(name, cig, start, bc, "U" + name, rn=rn, flag=16 if neg else 0, seq=seq, qual=qual, pre=pre))
        return cigar_table(start, cig), seq, qual, neg, bc, "U" + name, rn_value

    def ends(tab, k):
        return [tab[k][2], tab[k][2] + tab[k][1] - 1]

    start = 10_000_000
    # CIGARs of exactly n operations; where they exist, operations 62 .. 65 are M = X M: the two sides of the first round
    for idx, n_ops in enumerate(WALK_OPS):
        forced = {k: op for k, op in zip((62, 63, 64, 65), "M=XM") if k < n_ops}
        cig = gen_cigar(rng, n_ops, forced, {k: 3 for k in forced}) if n_ops > 1 else [("M", 40)]
        info = record(f"w{n_ops}", cig, start, neg=bool(idx & 1))
        tab = info[0]
        m_ops = [k for k, t in enumerate(tab) if t[0] in "M=X"]
        asked = []
        for k in sorted(set(list(forced) + m_ops[:2] + m_ops[-2:] + [int(x) for x in rng.choice(m_ops, min(6, len(m_ops)), replace=False)])):
            for which, p in zip(("first", "last"), ends(tab, k)):
                add(f"w{n_ops}_op{k}_{which}", [p], info, ops=[k])
                asked.append(p)
        good = [p for p in sorted(set(asked)) if lines[[ln["pos_text"] for ln in lines].index(str(p))]["ok"]]
        shuffled = [good[i] for i in rng.permutation(len(good))]
        add(f"w{n_ops}_all", shuffled, info, ops=[k for k in m_ops])                       # one walk for every position, across the rounds
        for k, t in enumerate(tab):                                                         # inside a deletion and an intron: no hit
            if t[0] in "DN" and k < 200:
                add(f"w{n_ops}_in{t[0]}{k}", [t[2] + t[1] // 2], info)
        dels = [t for t in tab if t[0] == "D"]
        if dels:                                                                            # only the last position in a deletion: nothing emitted
            before = [p for p in good if p < dels[-1][2]][:3]
            if before:
                add(f"w{n_ops}_lastdel", before + [dels[-1][2]], info)
        start += 1_000_000
    # the first base after an I, a D and an N that ends a round (operation 63 of round 0, 127 of round 1)
    for n_ops, at in ((129, 63), (300, 127)):
        for g in "IDN":
            cig = gen_cigar(rng, n_ops, {at - 1: "M", at: g, at + 1: "="})
            info = record(f"g{g.lower()}{n_ops}", cig, start, neg=g == "D")
            tab = info[0]
            add(f"after{g}{n_ops}_last_before", [ends(tab, at - 1)[1]], info, ops=[at - 1])
            add(f"after{g}{n_ops}_first", [ends(tab, at + 1)[0]], info, ops=[at + 1])
            add(f"after{g}{n_ops}_both", [ends(tab, at + 1)[0], ends(tab, at - 1)[1], ends(tab, at + 1)[1]], info, ops=[at - 1, at + 1])
            start += 1_000_000
    # an intron of 2^27 bases in the second round
    cig = gen_cigar(rng, 129, {69: "M", 70: "N", 71: "M"}, {70: 1 << 27})
    info = record("bign", cig, 50_000_000)
    tab = info[0]
    assert tab[-1][2] + tab[-1][1] < SNP_LN
    add("bign_before", [ends(tab, 69)[1]], info, ops=[69])
    add("bign_inside", [tab[70][2] + (1 << 26)], info)
    add("bign_after", [ends(tab, 71)[0]], info, ops=[71])
    last_m = [k for k, t in enumerate(tab) if t[0] in "M=X"][-1]
    add("bign_far", [ends(tab, 71)[0], ends(tab, 69)[0], ends(tab, last_m)[0]], info, ops=[69, 71, last_m])
    # the last base of the read is refused (readLength > max), the one in front of it is taken; the leading soft clip; in front of the start
    info = record("plain", [("M", 10)], 1000)
    add("plain_lastbase", [1009], info)
    add("plain_before_last", [1008], info, ops=[0])
    info = record("clipped", [("S", 5), ("M", 20), ("S", 1)], 2000)
    add("clip_under", [1998], info)
    add("clip_under_and_in", [1998, 2003], info)
    add("clip_before", [1990, 2001], info)
    add("clip_first", [2000], info, ops=[1])
    add("clip_last_m", [2019], info, ops=[1])
    # all sixteen base codes at even and at odd read offsets, on both strands
    codes = "=ACMGRSVTWYHKDBN"
    seq = codes + "N" + codes + "ACG"
    for neg, s in ((False, 3000), (True, 4000)):
        info = record("codes_r" if neg else "codes_f", [("M", 34), ("S", 2)], s, neg=neg, seq=seq, qual=bytes(range(10, 46)))
        for i in list(range(16)) + list(range(17, 33)):
            add(f"code{'r' if neg else 'f'}{i}", [s + i], info, ops=[0])
    # qualities against MINQV
    qual = bytes([0, 1, 99, 100, 101, 254, 50, 50, 50, 50, 50, 50])
    info = record("quals", [("M", 10), ("S", 2)], 5000, qual=qual)
    for i in range(6):
        add(f"q{qual[i]}", [5000 + i], info, ops=[0])
    add("q_pair", [5004, 5002], info, ops=[0])
    # RN of every integer type
    rns = [("c", 0), ("c", -5), ("c", 127), ("c", -128), ("C", 0), ("C", 127), ("C", 128), ("C", 255), ("s", -1), ("s", 128), ("s", 32767),
           ("s", -32768), ("S", 32767), ("S", 32768), ("S", 65535), ("i", 0), ("i", -7), ("i", 32768), ("i", 2 ** 31 - 1), ("I", 0),
           ("I", 32768), ("I", 2 ** 31 - 1)]
    for k, (code, v) in enumerate(rns):
        info = record(f"rn{k}", [("M", 20), ("S", 2)], 6000 + 100 * k, rn=tm.aux_int("RN", code, v), rn_value=v)
        add(f"rn_{code}_{v}", [6005 + 100 * k], info, ops=[0])
    # B arrays of every element type and an H attribute in front; BC, U8 and RN given twice: the last value counts
    pre = b"".join(tm.aux_b("X" + c, c, [1, 2, 3][:1 + i % 3]) for i, c in enumerate("cCsSiIf")) + tm.aux_b("XE", "S", []) + tm.aux_h("XH", "1AE301")
    pre += tm.aux_z("BC", "WRONGCELL") + tm.aux_z("U8", "WRONGUMI") + tm.aux_int("RN", "s", 300) + tm.aux_a("XA", "Z")
    info = record("twice", [("M", 20), ("S", 2)], 9000, rn=tm.aux_int("RN", "C", 9), rn_value=9, pre=pre)
    add("twice", [9003], info, ops=[0])
    order = rng.permutation(len(lines))
    lines = [lines[i] for i in order]
    return dict(bam=snp_bam([recs[i] for i in rng.permutation(len(recs))]), snp="".join(ln["text"] + "\n" for ln in lines),
                csv="".join(c + "\n" for c in cells), lines=lines)


def walk_expected(min_rn=0, min_qv=0):
    """(line_counts, molinfos text, row labels) of walk_case by construction: every line resolves on one record or on none"""
    counts, mol, rows = [], [], set()
    for ln in walk_case()["lines"]:
        c = dict(line=ln["text"], hits=0, lowRN=0, lowQV=0)
        if ln["ok"]:
            if ln["rn"] < min_rn:
                c["lowRN"] = 1
            elif min(ln["quals"] + [100]) < min_qv:
                c["lowQV"] = 1
            else:
                c["hits"] = 1
                tx = f"chr1:{ln['pos_text']}..{ln['bases']}"
                rows.add(f"{ln['gene']}\t{tx}")
                mol.append(f"{ln['bc']}\t{ln['umi']}\t{ln['rn'] if ln['rn'] > 1 else 1}\t0\tnull\t{','.join(map(str, ln['quals']))}\t{ln['gene']}\t{tx}\n")
        counts.append(c)
    return counts, (MOLHEAD + "".join(mol)).encode("latin-1"), sorted(rows, key=str.encode)


# (MINRN, MINQV) of the walk runs: MINQV on both sides of every quality with MINRN 0 (RN is tested first: the quality lines have RN 1),
# MINRN on both sides of every RN with MINQV 0, and both filters at once
WALK_FILTERS = ((0, 0), (0, 1), (0, 2), (0, 99), (0, 100), (0, 101), (0, 102), (0, 254), (0, 255),
                (1, 0), (127, 0), (128, 0), (129, 0), (32767, 0), (32768, 0), (32769, 0), (-200, 0), (128, 100), (1, 99))

SNP_CASES = dict(render=render_case, wide=wide_case, search=search_case, table=table_case, walk=walk_case)


# ---- (d) K-ISO -------------------------------------------------------------------------------------------------------------------------
ISO_HEAD = "@HD\tVN:1.6\n@SQ\tSN:chr12\tLN:100000000\n"
ISO_REFS = [("chr12", 100000000)]
LDS_TX = 64                     # the lds_tx the GPU test runs with: G64 stays in LDS, G65 spills
GENE_SIZES = (1, 63, 64, 65, 200)


def tx_line(gene, tx, junc, start=None):
    """a refFlat line whose junctions (exon end, next exon start; 1-based) are `junc`; without junctions one exon at start"""
    if not junc:
        xs, xe = [start], [start + 500]
    else:
        xs = [junc[0][0] - 100] + [e - 1 for _s, e in junc]
        xe = [s for s, _e in junc] + [junc[-1][1] + 100]
    return (f"{gene}\t{tx}\tchr12\t+\t{xs[0]}\t{xe[-1]}\t{xs[0]}\t{xe[-1]}\t{len(xs)}\t" + "".join(f"{x}," for x in xs) + "\t"
            + "".join(f"{x}," for x in xe) + "\n")


def cigar_for(junc, shift=(0, 0)):
    """(pos0, M / N operations) of a read whose junctions are `junc`, every junction start / end moved by shift"""
    pos1 = junc[0][0] - 40 if junc else None
    cig, cur = [], pos1
    for s, e in junc:
        s, e = s + shift[0], e + shift[1]
        cig += [("M", s - cur + 1), ("N", e - s - 1)]
        cur = e
    return pos1 - 1, cig + [("M", 30)]


def gene_junc(base, t):
    return [(base + 100, base + 1001 + 10 * t), (base + 1100 + 10 * t, base + 5001)]


def chain_junc(base, n):
    return [(base + 100 + 200 * i, base + 201 + 200 * i) for i in range(n)]


def irec(name, cigar, pos0, bc, umi, gene):
    aux = tm.aux_z("BC", bc) + tm.aux_z("U8", umi) + tm.aux_z("GE", gene)
    return bammodel.bam_record(name, 0, 0, pos0, 60, cigar, "ACGT", aux=aux)


GENE_CELLS = 66
GENE_COUNTS = {0: 1001, 1: 9, 62: 99, 63: 10, 64: 101}      # GA's molecules per cell K000 .. K065 (the last column: no hit)


@functools.lru_cache(maxsize=None)
def iso_case():
    """-> dict(bam, refflat, csv, expect: {(cell, umi): (gene, transcript, supporting records)} at delta 2, n_t: {(cell, umi): candidate
    transcripts}, n_rec: {(cell, umi): records}, n_junc: junction counts of the reads)"""
    rng = np.random.default_rng(404)
    ref, recs, expect, n_t, n_rec = [], [], {}, {}, {}
    base = {}
    at = 100000

    def gene(name, n, tx_name=None, junc=None):
        nonlocal at
        base[name] = at
        for t in range(n):
            ref.append(tx_line(name, tx_name(t) if tx_name else f"{name}T{t:03d}", junc(at, t) if junc else gene_junc(at, t), start=at))
        at += 20000

    def mol(cell, umi, genes, reads, want, nt):
        """reads: [(junctions, shift)], one record each"""
        for i, (junc, shift) in enumerate(reads):
            if junc:
                p0, cig = cigar_for(junc, shift)
            else:
                p0, cig = shift, [("M", 40)]
            recs.append(irec(f"{cell}_{umi}_{i}", cig, p0, cell, umi, genes))
        expect[(cell, umi)] = want
        n_t[(cell, umi)] = nt
        n_rec[(cell, umi)] = len(reads)

    for n in GENE_SIZES:
        gene(f"G{n}", n)
    b = base
    # candidate sets of LDS_TX and LDS_TX + 1 lines side by side in one block (molecules 0 and 1), the match on the last line of each
    mol("S000", "lds", "G64", [(gene_junc(b["G64"], 63), (0, 0))], ("G64", "G64T063", 1), 64)
    mol("S000", "spill", "G65", [(gene_junc(b["G65"], 64), (0, 0))], ("G65", "G65T064", 1), 65)
    # molecules of 63, 64, 65 and 200 records; candidate sets of 1, 63, 65 and 200 lines
    mol("S001", "r63", "G1", [(gene_junc(b["G1"], 0), (1, -1))] * 63, ("G1", "G1T000", 63), 1)
    mol("S001", "r64", "G63", [(gene_junc(b["G63"], 62), (0, 2))] * 64, ("G63", "G63T062", 64), 63)
    mol("S002", "r65", "G200", [(gene_junc(b["G200"], 150), (0, 0))] * 33 + [(gene_junc(b["G200"], 199), (0, 0))] * 32, ("G200", "G200T150", 33), 200)
    mol("S002", "r200", "G200", [(gene_junc(b["G200"], 130 if i % 2 else 70), (0, 0)) for i in range(200)], ("G200", "G200T070", 100), 200)
    mol("S003", "two_genes", "G65,G200", [(gene_junc(b["G200"], 199), (2, 2))], ("G200", "G200T199", 1), 265)
    # a tie among 130 lines of the same junctions: the smallest key is line 100, in the second batch of 64
    gene("GT", 130, tx_name=lambda t: "A000" if t == 100 else f"T{999 - t}", junc=lambda a, t: gene_junc(a, 0))
    mol("S004", "tie130", "GT", [(gene_junc(b["GT"], 0), (0, 0))] * 2, ("GT", "A000", 2), 130)
    # no match and a tie among 70 genes of two lines each: the gene whose first refFlat line comes first
    for g in range(70):
        gene(f"NM{g:02d}", 2)
    nm = [f"NM{g:02d}" for g in range(70)]
    mol("S005", "nomatch70", ",".join(nm[i] for i in rng.permutation(70)), [(gene_junc(b["NM33"], 7), (0, 0))], ("NM00", "undef", 0), 140)
    gene("NM3", 3)                                           # three lines beat two, wherever the gene stands in the attribute
    mol("S005", "nomatch_most", ",".join(nm[40:] + ["NM3"] + nm[:40]), [(gene_junc(b["NM33"], 7), (0, 0))], ("NM3", "undef", 0), 143)
    # reads of 0, 1, 64 and 65 junctions
    gene("MONO", 1, junc=lambda a, t: [])
    mol("S006", "mono", "MONO", [([], base["MONO"] + 10)], ("MONO", "MONOT000", 1), 1)
    mol("S006", "j0", "G63", [([], b["G63"] + 10)], ("G63", "undef", 0), 63)
    gene("J1", 1, junc=lambda a, t: chain_junc(a, 1))
    mol("S006", "j1", "J1", [(chain_junc(b["J1"], 1), (-2, 2))], ("J1", "J1T000", 1), 1)
    gene("J64", 2, junc=lambda a, t: chain_junc(a, 64 + t))
    mol("S006", "j64", "J64", [(chain_junc(b["J64"], 64), (0, 0))], ("J64", "J64T000", 1), 2)
    mol("S006", "j65", "J64", [(chain_junc(b["J64"], 65), (0, 0))] * 2, ("J64", "J64T001", 2), 2)
    mol("S006", "j63", "J64", [(chain_junc(b["J64"], 63), (0, 0))], ("J64", "undef", 0), 2)
    # reads one and two bases off: matched at delta 2, not at delta 0
    mol("S007", "off1", "G63", [(gene_junc(b["G63"], 10), (1, 0))], ("G63", "G63T010", 1), 63)
    mol("S007", "off3", "G63", [(gene_junc(b["G63"], 11), (3, 0))], ("G63", "undef", 0), 63)
    n_special = len(recs)
    # the gene matrix: GENE_COUNTS molecules of GA per cell, 1 to 3 reads each, the repeats in the tail of the file
    gene("GA", 1)
    first, tail = [], []
    for k, n in GENE_COUNTS.items():
        for j in range(n):
            for t in range(int(rng.integers(1, 4))):
                p0, cig = cigar_for(gene_junc(b["GA"], 0))
                (tail if t else first).append(irec(f"ga{k}_{j}_{t}", cig, p0, f"K{k:03d}" + ("-1" if j % 2 else ""), f"U{j:05d}", "GA"))
    recs += [first[i] for i in rng.permutation(len(first))] + [tail[i] for i in rng.permutation(len(tail))]
    cells = sorted({c for c, _u in expect} | {f"K{k:03d}" for k in range(GENE_CELLS)})
    return dict(bam=bammodel.bam_bytes(ISO_HEAD, ISO_REFS, recs), refflat="".join(ref), csv="".join(c + "\n" for c in cells), cells=cells,
                expect=expect, n_t=n_t, n_rec=n_rec, n_special=n_special)


def gene_matrix_row(cells):
    """GA's row of the gene matrix by construction"""
    return "GA" + "".join(f"\t{GENE_COUNTS.get(int(c[1:]), 0) if c[0] == 'K' else 0}" for c in cells) + "\n"


@functools.lru_cache(maxsize=None)
def iso_model(delta=2, isobam=False):
    c = iso_case()
    return im.isoform_matrix(c["bam"], c["refflat"], c["csv"], delta=delta, isobam=isobam)
