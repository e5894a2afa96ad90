"""The inputs of tests/test_bamindex_cpu.py and tests/test_bamindex_gpu.py: BAM files built from literals and seeds with bammodel's writer,
the BGZF blocks cut where each case wants them.  A case is (file bytes, segment_bytes of the segmented run).  Test infrastructure only."""
import random

import bammodel

HEAD = "@HD\tVN:1.6\tSO:coordinate\n"
BIG = 1 << 29
OPS = "MIDNSHP=X"


def rec(name, ref, pos, cigar, flag=0, seq="ACGT", aux=b""):
    return bammodel.bam_record(name, flag, ref, pos, 30, cigar, seq, aux=aux)


def unplaced(name):
    return rec(name, -1, -1, [], flag=4)


def header(refs, head=HEAD):
    return bammodel.bam_bytes(head + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs), refs, [])


def cut_blocks(data, cuts, eof=True, empty_at=()):
    """the BGZF file whose blocks end at the inflated positions `cuts` (and at the end); empty_at: positions of `cuts` (or 0) in front of
    which an empty block stands"""
    edges = sorted(set([0] + [c for c in cuts if 0 < c < len(data)] + [len(data)]))
    out = []
    for a, b in zip(edges, edges[1:]):
        if a in empty_at:
            out.append(bammodel.bgzf_block(b""))
        out.append(bammodel.bgzf_block(data[a:b]))
    if eof:
        out.append(bammodel.bgzf_block(b""))
    return b"".join(out)


def file_of(refs, records, block=0xFF00, eof=True):
    data = header(refs) + b"".join(records)
    return cut_blocks(data, range(block, len(data), block), eof=eof)


def small(raw, parts=6):
    return max(32, len(raw) // parts)


def cigar_of(n, seed):
    """n operations over all nine kinds, lengths 1 .. 3"""
    rng = random.Random(seed)
    return [(OPS[(k + seed) % 9], 1 + rng.randrange(3)) for k in range(n)]


# ---- the hand-built file: tests/test_bamindex_cpu.py writes its .bai out byte by byte ----------------------------------------------------
def hand():
    """header 50 bytes, then records of 57, 50 and 41 bytes; blocks of inflated bytes [0, 100), [100, 160) and [160, 198)"""
    refs = [("chr1", 100000)]
    data = bammodel.bam_bytes(HEAD, refs, [rec("a", 0, 100, [("M", 10)], seq="ACGTACGTAC"), rec("b", 0, 20000, [("M", 5)], seq="ACGTA"),
                                           rec("c", -1, -1, [], flag=4, seq="AC")])
    assert len(data) == 198
    return cut_blocks(data, [100, 160]), 40


# ---- extents and bins ---------------------------------------------------------------------------------------------------------------------
def extents():
    R = []
    for k, n in enumerate((0, 1, 63, 64, 65, 300, 65535)):
        R.append((10 + k, f"ops{n}", cigar_of(n, k), 0))
    R.append((30, "onlySI", [("S", 5), ("I", 3)], 0))
    R.append((31, "placed4", [("M", 50)], 4))
    R.append((32, "cgplaceholder", [("S", 4), ("N", 5000)], 0))
    for k in (14, 17, 20, 23, 26):
        R.append(((1 << k) - 10, f"ends_on_2^{k}", [("M", 10)], 0))          # end = 2^k: stays in the lower bin
        R.append(((1 << k) - 5, f"across_2^{k}", [("M", 10)], 0))
    R.append(((1 << 27) + 3, "skip_2^27", [("M", 5), ("N", 1 << 27), ("M", 5)], 0))
    R.append((BIG - 100, "end_2^29", [("M", 100)], 0))
    R.append((BIG - 1, "pos_2^29-1", [("M", 1)], 0))
    R += [(1000 + 53 * k, f"fill{k}", [("M", 20 + k % 7)], 0) for k in range(600)]     # so that the segmented run has segments to cut
    R.sort(key=lambda r: r[0])
    raw = file_of([("big", BIG)], [rec(nm, 0, pos, cg, flag) for pos, nm, cg, flag in R], block=4096)
    return raw, 2000


# ---- offsets ------------------------------------------------------------------------------------------------------------------------------
def offsets(border=False):
    """record 0 fills a block of its own behind a block that holds the header alone; record 1 (a CIGAR of 300 operations) spans three blocks;
    an empty block stands behind record 2; then 240 records in blocks of 150 bytes; no EOF block.  border: the segmented run's first
    segment ends exactly in front of the empty block, behind record 2"""
    refs = [("chr1", 1 << 20)]
    H = header(refs)
    R = [rec("fills", 0, 5, [("M", 20)]), rec("spans3", 0, 6, cigar_of(300, 3)), rec("before_empty", 0, 7, [("M", 9)])]
    R += [rec(f"r{k}", 0, 100 + 37 * k, [("M", 30 + k)]) for k in range(240)]
    data = H + b"".join(R)
    a = len(H) + len(R[0])
    e = a + len(R[1]) + len(R[2])
    cuts = [len(H), a, a + 400, a + 900, e] + list(range(e + 150, len(data), 150))
    raw = cut_blocks(data, cuts, eof=False, empty_at=(e,))
    if not border:
        return raw, small(raw, 7)
    first = sum(len(bammodel.bgzf_block(data[x:y])) for x, y in zip([0] + cuts[:4], cuts[:5]))
    assert first * 4 <= len(raw)
    return raw, first


# ---- chunks -------------------------------------------------------------------------------------------------------------------------------
def chunks():
    """the first and the last record lie in bin 0; runs of 1, 2, 63, 64 and 65 records in the windows 1 .. 5; bins A B A B over 130 records in
    window 10; one run of 3000 records in window 20"""
    refs = [("chr1", 1 << 28)]
    R = [rec("first_bin0", 0, 0, [("M", 1), ("N", 1 << 26), ("M", 1)])]
    for w, n in enumerate((1, 2, 63, 64, 65), start=1):
        R += [rec(f"run{n}_{j}", 0, (w << 14) + j, [("M", 8)]) for j in range(n)]
    for j in range(130):
        R.append(rec(f"abab{j}", 0, (10 << 14) + j, [("M", 4)] if j % 2 == 0 else [("M", 20000)]))
    R += [rec(f"long{j}", 0, (20 << 14) + j, [("M", 8)]) for j in range(3000)]
    R.append(rec("last_bin0", 0, (1 << 26) - 1, [("M", 2)]))
    raw = file_of(refs, R, block=3000)
    return raw, small(raw, 8)


# ---- references ---------------------------------------------------------------------------------------------------------------------------
def no_references():
    raw = file_of([], [], block=64)
    return raw, 32


def only_unplaced():
    raw = file_of([("chr1", 1000), ("chr2", 1000)], [unplaced(f"u{k}") for k in range(40)], block=200)
    return raw, small(raw)


def many_references():
    """3,000 references of which every third has records; the first and the last have none"""
    refs = [(f"c{r}", 40000) for r in range(3000)]
    R = []
    for r in range(1, 3000, 3):
        R += [rec(f"c{r}a", r, 10, [("M", 5)]), rec(f"c{r}b", r, 20000, [("M", 5)])]
    raw = file_of(refs, R, block=5000)
    return raw, small(raw, 16)


# ---- linear index -------------------------------------------------------------------------------------------------------------------------
def linear():
    """windows 0 .. 4 empty, a gap of 10 windows (6 .. 15), and the record of 8,193 windows"""
    refs = [("chr1", BIG)]
    R = [rec("w5", 0, (5 << 14) + 7, [("M", 10)]), rec("w16", 0, (16 << 14) + 1, [("M", 10)])]
    R += [rec(f"w17_{k}", 0, (17 << 14) + k, [("M", 10)]) for k in range(40)]
    R.append(rec("windows8193", 0, (100 << 14) + 16000, [("M", 5), ("N", 1 << 27), ("M", 5)]))
    R += [rec(f"tail{k}", 0, (200 << 14) + k, [("M", 10)]) for k in range(40)]
    raw = file_of(refs, R, block=500)
    return raw, small(raw)


# ---- stops: name -> (file, segment_bytes, record, read, the model's kind) ------------------------------------------------------------------
def _stop_file(records, border_at=None):
    """border_at: the segmented run's first segment ends behind record border_at - 1"""
    refs = [("chr1", BIG), ("chr2", BIG)]
    H = header(refs)
    data = H + b"".join(records)
    if border_at is None:
        raw = cut_blocks(data, range(300, len(data), 300))
        return raw, small(raw)
    e = len(H) + sum(len(r) for r in records[:border_at])
    cuts = sorted(set(list(range(300, e, 300)) + [e] + list(range(e + 300, len(data), 300))))
    raw = cut_blocks(data, cuts)
    first = sum(len(bammodel.bgzf_block(data[x:y])) for x, y in zip([0] + cuts, cuts) if y <= e)
    assert first * 4 <= len(raw)
    return raw, first


def stops():
    def base(ref=0):
        return [rec(f"s{k}", ref, 1000 + 10 * k, [("M", 50)]) for k in range(30)]
    out = {}
    R = base() + [rec("back", 0, 1200, [("M", 50)])] + [rec(f"t{k}", 0, 2000 + k, [("M", 5)]) for k in range(120)]
    out["pos_decreases_inside"] = _stop_file(R) + (30, "back", "order")
    out["pos_decreases_at_border"] = _stop_file(R, border_at=30) + (30, "back", "order")
    R = base(1) + [rec("ref_back", 0, 5000, [("M", 50)])] + [rec(f"t{k}", 1, 9000 + k, [("M", 5)]) for k in range(120)]
    out["ref_decreases"] = _stop_file(R) + (30, "ref_back", "order")
    R = base() + [unplaced("u0"), rec("behind_unplaced", 1, 5, [("M", 5)])] + [unplaced(f"v{k}") for k in range(120)]
    out["placed_behind_unplaced"] = _stop_file(R) + (31, "behind_unplaced", "order")
    R = [rec("negative", 0, -1, [("M", 5)])] + base() + [rec(f"t{k}", 0, 2000 + k, [("M", 5)]) for k in range(120)]
    out["negative_pos"] = _stop_file(R) + (0, "negative", "negative")
    R = base() + [rec("too_far", 0, BIG - 10, [("M", 11)])] + [rec(f"t{k}", 1, 2000 + k, [("M", 5)]) for k in range(120)]
    out["end_2^29+1"] = _stop_file(R) + (30, "too_far", "far")
    return out


# ---- seeded -------------------------------------------------------------------------------------------------------------------------------
def seeded(seed=7, n=20000, n_unplaced=300):
    rng = random.Random(seed)
    refs = [(f"chr{r + 1}", 50_000_000) for r in range(5)]
    keys = sorted((rng.randrange(5), rng.randrange(40_000_000)) for _ in range(n))
    R = []
    for k, (ref, pos) in enumerate(keys):
        kind = rng.randrange(10)
        cg = [("M", 1 + rng.randrange(2000))]
        if kind < 4:
            cg += [("N", 1 + rng.randrange(100000)), ("M", 1 + rng.randrange(500))]
        if kind == 9:
            cg = cigar_of(1 + rng.randrange(80), k)
        R.append(rec(f"q{k}", ref, pos, cg, flag=4 if rng.randrange(200) == 0 else 0))
    R += [unplaced(f"un{k}") for k in range(n_unplaced)]
    return file_of(refs, R, block=0xFF00)


def random_regions(raw_refs, n=200, seed=11):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        ref = rng.randrange(len(raw_refs))
        beg = rng.randrange(max(1, min(raw_refs[ref][1], 40_000_000)))
        out.append((ref, beg, beg + 1 + rng.randrange(1 << rng.randrange(1, 22))))
    return out


# ---- the writers' input: names of the molecule form, two references, unplaced records last ------------------------------------------------
def writer_names(n=600):
    return [f"ACGTACGTACGTACGT-TTTTGGGGCCCC-{k}" for k in range(n)]


def writer_input(unsorted=False, with_unplaced=True):
    refs = [("chr1", 1 << 20), ("chr2", 1 << 20)]
    names = writer_names()
    R = [rec(nm, k // 300, 500 + 97 * (k % 300), [("M", 40), ("N", 700), ("M", 40)], seq="ACGTACGTAC") for k, nm in enumerate(names)]
    if unsorted:
        R[200], R[450] = R[450], R[200]
    if with_unplaced:
        R += [unplaced(f"ACGTACGTACGTACGT-TTTTGGGGCCCC-{9000 + k}") for k in range(5)]
    return refs, file_of(refs, R, block=2000)


def writer_fastq():
    return "".join(f"@{nm}\nACGTACGTAC\n+\nIIIIIIIIII\n" for nm in writer_names() + [f"ACGTACGTACGTACGT-TTTTGGGGCCCC-{9000 + k}" for k in range(5)]).encode()


WRITER_REFFLAT = "GENE1\tTX1\tchr1\t+\t400\t40000\t400\t40000\t2\t400,20000,\t10000,40000,\n"

CASES = dict(hand=hand, extents=extents, offsets=offsets, offsets_border=lambda: offsets(border=True), chunks=chunks, no_references=no_references,
             only_unplaced=only_unplaced, many_references=many_references, linear=linear)
