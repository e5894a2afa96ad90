"""The inputs of tests/test_bamview_cpu.py and tests/test_bamview_gpu.py: BAM files built from literals and seeds with bammodel's writer,
their index from baimodel.bai_model, and the foreign-form index made from it.  A case is (file bytes, segment_bytes of the segmented run,
regions or None, filters).  tests/test_bamview_cpu.py asserts the edges named here.  Test infrastructure only."""
import random
import struct

import baicases as bc
import baimodel as bm
import bammodel
import sortcases

HEAD = bc.HEAD
INTERVAL_COUNTS = (1, 2, 63, 64, 65, 1000)
CIGAR_COUNTS = (0, 1, 15, 16, 17, 33, 1000)
LENGTHS = (37, 63, 64, 65, 255, 256, 257, 70000)


def rec(name, ref, pos, cigar=(("M", 10),), flag=0, mapq=30, seq="ACGT", aux=b""):
    return bammodel.bam_record(name, flag, ref, pos, mapq, list(cigar), seq, aux=aux)


# ---- the foreign-form index ----------------------------------------------------------------------------------------------------------------
def coalesce(chunks):
    out = []
    for b, e in sorted(chunks):
        if out and b <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((b, e))
    return out


def foreign_bai(parsed, occupied):
    """an index another writer could have left for the same file, from a parsed canonical one (baimodel.parse_bai's first part): every
    level-5 bin folded into its parent with the chunk lists sorted and coalesced, the linear windows without a record (occupied: per
    reference the set of windows with one) filled backwards from the next one that has one, no pseudo-bin and no trailing n_no_coor"""
    out = [b"BAI\x01", struct.pack("<i", len(parsed))]
    for r, occ in zip(parsed, occupied):
        bins = {}
        for b, chunks in r["bins"].items():
            bins.setdefault((b - 1) >> 3 if b >= 4681 else b, []).extend(chunks)
        out.append(struct.pack("<i", len(bins)))
        for b in sorted(bins, reverse=True):                 # bins in an order of its own
            ch = coalesce(bins[b])
            out.append(struct.pack("<Ii", b, len(ch)) + b"".join(struct.pack("<QQ", *c) for c in ch))
        lin = list(r["lin"])
        for w in range(len(lin) - 2, -1, -1):
            if w not in occ:
                lin[w] = lin[w + 1]
        out.append(struct.pack("<i", len(lin)) + b"".join(struct.pack("<Q", v) for v in lin))
    return b"".join(out)


def indexes(raw):
    """-> (this build's canonical .bai, the foreign-form one) of a coordinate-sorted file"""
    ours = bm.bai_model(raw)
    refs, recs = bm.records_of(raw)
    occupied = [set() for _ in refs]
    for ref, beg, end, _flag, _vb, _ve, _name in recs:
        if ref >= 0:
            occupied[ref].update(range(beg >> 14, ((end - 1) >> 14) + 1))
    return ours, foreign_bai(bm.parse_bai(ours)[0], occupied)


# ---- 1. the hand-built file ----------------------------------------------------------------------------------------------------------------
def hand():
    """six records: a (chr1 100..110), b (chr1 105..106, flag 0x4 with a CIGAR of 50), c (chr1 20000..20005, mapq 5), d (chr2 7..17,
    reverse), e (chr2 16..17, no CIGAR), u (unplaced); the region chr1:101-110 and chr2:17"""
    refs = [("chr1", 100000), ("chr2", 1000)]
    R = [rec("a", 0, 100), rec("b", 0, 105, [("M", 50)], flag=4), rec("c", 0, 20000, [("M", 5)], mapq=5), rec("d", 1, 7, flag=16),
         rec("e", 1, 16, []), bc.unplaced("u")]
    return bc.file_of(refs, R, block=120), 64, ["chr1:101-110", "chr2:17"], {}


# ---- 2. extents against region borders -----------------------------------------------------------------------------------------------------
def borders():
    """CIGARs of 0, 1, 15, 16, 17, 33 and 1,000 operations over all nine letters; around the region [5000, 6000): a record that ends at
    5000 (out) and at 5001 (in), one at 5999 (in) and one at 6000 (out); a placed flag-0x4 record with a CIGAR of 300 bases that ends, as
    one base, in front of the region; records whose reference length is 0 (S and I alone)"""
    R = []
    for k, n in enumerate(CIGAR_COUNTS):
        R.append((4000 + 40 * k, f"ops{n}", bc.cigar_of(n, k), 0))
    R += [(4990, "ends_at_beg", [("M", 10)], 0), (4991, "one_base_in", [("M", 5), ("D", 2), ("N", 2), ("=", 1)], 0), (4800, "flag4_long", [("M", 300)], 4),
          (4999, "SI_before", [("S", 5), ("I", 3)], 0), (5000, "SI_first_base", [("S", 5), ("I", 3)], 0), (5999, "last_base", [("M", 10)], 0),
          (6000, "at_end", [("M", 10)], 0), (5500, "inside", [("X", 3)], 0), (3000, "across", [("M", 10), ("N", 5000), ("M", 10)], 0)]
    R += [(100 + 61 * k, f"fill{k}", [("M", 20 + k % 7)], 0) for k in range(150)]
    R.sort(key=lambda r: r[0])
    raw = bc.file_of([("chr1", 1 << 20)], [rec(nm, 0, pos, cg, flag) for pos, nm, cg, flag in R], block=1500)
    return raw, bc.small(raw, 8), [(0, 5000, 6000)], {}


# ---- 3. many intervals ---------------------------------------------------------------------------------------------------------------------
def intervals():
    """references with 1, 2, 63, 64, 65 and 1,000 merged intervals [100 k + 10, 100 k + 20): records in front of the first, inside each,
    between each pair and behind the last"""
    refs = [(f"r{n}", 1 << 20) for n in INTERVAL_COUNTS]
    R, regions = [], []
    for ref, n in enumerate(INTERVAL_COUNTS):
        R.append(rec(f"r{n}_front", ref, 0, [("M", 10)]))
        for k in range(n):
            R.append(rec(f"r{n}_in{k}", ref, 100 * k + 5, [("M", 6)]))           # ends at 100 k + 11: one base in
            R.append(rec(f"r{n}_gap{k}", ref, 100 * k + 20, [("M", 90)]))         # [100 k + 20, 100 k + 110): touches both neighbours, in neither
            regions.append((ref, 100 * k + 10, 100 * k + 20))
    random.Random(5).shuffle(regions)
    raw = bc.file_of(refs, R, block=6000)
    return raw, bc.small(raw, 8), regions, {}


# ---- 4. regions that merge -----------------------------------------------------------------------------------------------------------------
def merging():
    """overlapping ([100, 200) and [150, 300)) and touching ([300, 400)) regions become one; `both` overlaps [100, 400) and [1000, 1100)
    and is written once; the same region twice"""
    R = [rec("before", 0, 50, [("M", 50)]), rec("first", 0, 120), rec("seam", 0, 299, [("M", 2)]), rec("both", 0, 390, [("M", 5), ("N", 700), ("M", 5)]),
         rec("between", 0, 500), rec("second", 0, 1050), rec("after", 0, 1100)]
    R += [rec(f"fill{k}", 0, 2000 + 13 * k) for k in range(200)]
    raw = bc.file_of([("chr1", 1 << 20)], R, block=700)
    return raw, bc.small(raw), ["chr1:101-200", "chr1:151-300", "chr1:301-400", (0, 1000, 1100), ("chr1", 1000, 1100)], {}


# ---- 5. references -------------------------------------------------------------------------------------------------------------------------
def many_references():
    """3,000 references, records on the first, on every third and on the last; the regions name the first, the last and c2, which has no
    record"""
    refs = [(f"c{r}", 40000) for r in range(3000)]
    R = [rec("first_ref", 0, 7)]
    for r in range(1, 2999, 3):
        R += [rec(f"c{r}a", r, 10, [("M", 5)]), rec(f"c{r}b", r, 20000, [("M", 5)])]
    R += [rec("last_ref_a", 2999, 7), rec("last_ref_b", 2999, 30000)]
    raw = bc.file_of(refs, R, block=5000)
    return raw, bc.small(raw, 16), ["c0", "c2999:30,001", "c2"], {}


def nothing():
    raw = borders()[0]
    return raw, bc.small(raw, 8), [(0, 900000, 900010)], {}


def everything():
    raw = borders()[0]
    return raw, bc.small(raw, 8), ["chr1"], {}


# ---- 6. the gather -------------------------------------------------------------------------------------------------------------------------
def alignments():
    """sortcases.alignments' construction, sorted: 3,000 records whose lengths step from 37 bytes up; flag 0x400 on a seeded third, which
    -F 0x400 drops: the kept records' (offset in the segment mod 16, offset in the output mod 16) take all 256 values.  No region."""
    rng = random.Random(3)
    R = [sortcases.sized(k, 37 + k % 48, 0, 10 * k, flag=0x400 if rng.randrange(3) == 0 else 0, rng=rng) for k in range(3000)]
    raw = bc.file_of([("chr1", 1 << 20)], R, block=5000)
    return raw, bc.small(raw), None, dict(exclude=0x400)


def lengths():
    """records of 37, 63, 64, 65, 255, 256, 257 and 70,000 bytes inside the region, one of each outside"""
    R = [sortcases.sized(k, n, 0, 1000 + 10 * k) for k, n in enumerate(LENGTHS)] + [sortcases.sized(50 + k, n, 0, 5000 + 10 * k) for k, n in enumerate(LENGTHS)]
    raw = bc.file_of([("chr1", 1 << 20)], R, block=4000)
    return raw, bc.small(raw, 12), ["chr1:1,001-2,000"], {}


# ---- 7. the filters ------------------------------------------------------------------------------------------------------------------------
def filters():
    """-f 0x3 -F 0x900 -q 20: both required bits, one missing, the other missing; one excluded bit present, the other; mapq 20 and 19"""
    R = [rec("keep", 0, 100, flag=0x3), rec("keep_more_bits", 0, 110, flag=0x3 | 0x10 | 0x40), rec("bit1_missing", 0, 120, flag=0x2),
         rec("bit2_missing", 0, 130, flag=0x1), rec("excluded_0x100", 0, 140, flag=0x3 | 0x100), rec("excluded_0x800", 0, 150, flag=0x3 | 0x800),
         rec("mapq_at", 0, 160, flag=0x3, mapq=20), rec("mapq_below", 0, 170, flag=0x3, mapq=19), rec("mapq_255", 0, 180, flag=0x3, mapq=255),
         rec("outside", 0, 5000, flag=0x3)]
    R += [rec(f"fill{k}", 0, 6000 + 13 * k, flag=0x3 if k % 2 else 0) for k in range(100)]
    raw = bc.file_of([("chr1", 1 << 20)], R, block=500)
    return raw, bc.small(raw), ["chr1:1-1000", "chr1:6,001"], dict(require=0x3, exclude=0x900, min_mapq=20)


def unsorted_no_region():
    """sortcases.hand: unsorted, with unplaced records and a negative ref_id; -F 4 drops the flag-0x4 ones"""
    raw, seg, _window = sortcases.hand()
    return raw, seg, None, dict(exclude=4)


CASES = dict(hand=hand, borders=borders, intervals=intervals, merging=merging, many_references=many_references, nothing=nothing, everything=everything,
             alignments=alignments, lengths=lengths, filters=filters, unsorted_no_region=unsorted_no_region)


def regions_of(raw, regions):
    """the case's regions as (ref_id, beg, end), by the model's grammar"""
    import viewmodel as vm
    names = [n for n, _l in bammodel.parse_bam(bammodel.bgzf_decompress(raw))[1]]
    if regions is None:
        return None
    return [vm.parse_region(r, names) if isinstance(r, str) else (names.index(r[0]) if isinstance(r[0], str) else r[0], r[1], min(r[2], vm.MAX_END))
            for r in regions]


# ---- 8. seeded -----------------------------------------------------------------------------------------------------------------------------
def seeded():
    """baicases.seeded: 20,000 sorted records over 5 references and 300 unplaced -> (raw, 1,000 seeded regions)"""
    raw = bc.seeded()
    refs = [(f"chr{r + 1}", 50_000_000) for r in range(5)]
    return raw, bc.random_regions(refs, n=1000, seed=29)


# ---- 9. stops ------------------------------------------------------------------------------------------------------------------------------
def stop_ref():
    """record 25 has ref_id = n_ref, record 31 a larger one: the first is named.  Sorted, so that an index-free run reaches it in file
    order -> (raw, segment_bytes, record, read)"""
    R = [rec(f"s{k}", 0, 10 * k) for k in range(40)]
    R[25] = rec("beyond", 2, 5)
    R[31] = rec("further", 9, 5)
    raw = sortcases.file_of([("chr1", 1 << 20), ("chr2", 1 << 20)], R, block=300)
    return raw, sortcases.small(raw), 25, "beyond"


def mid_record_index(raw):
    """the canonical index of raw with the begin of the first chunk of its first reference moved 5 bytes on: into the record"""
    parsed, _no_coor = bm.parse_bai(bm.bai_model(raw))
    first = min(c[0] for ch in parsed[0]["bins"].values() for c in ch)
    out = bytearray(bm.bai_model(raw))
    at = out.find(struct.pack("<Q", first), 8)
    out[at:at + 8] = struct.pack("<Q", first + 5)
    return bytes(out)


def three_chromosomes():
    """the layout of tests/test_assignumis_shards_gpu.py's input: chr1, chr2 and chr3 of 10^6 bases, reads at twelve loci each in
    coordinate order, four unmapped records last, blocks of 4,096 bytes"""
    rng = random.Random(71)
    rows = sorted((m % 3, 30_000 + 4_000 * (m // 3 % 12) + rng.randrange(80), f"read{m}_{c}", 16 if m & 1 else 0, 200 + rng.randrange(300))
                  for m in range(90) for c in range(4))
    refs = [("chr1", 10 ** 6), ("chr2", 10 ** 6), ("chr3", 10 ** 6)]
    R = [bammodel.bam_record(nm, fl, ref, p0, 30, [("M", L)], "C" * L) for ref, p0, nm, fl, L in rows]
    R += [bammodel.bam_record(f"unmapped{k}", 4, -1, -1, 0, [], "C" * 300) for k in range(4)]
    return bc.file_of(refs, R, block=4096), refs
