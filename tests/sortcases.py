"""The inputs of the BamSort tests, built from literals and seeds with bammodel's writer.  A case is (the BAM file's bytes, segment_bytes,
window_bytes): the sizes of its segmented run (four or more segments, windows of a few kilobytes); every case also runs in one segment and
one window.  tests/test_bamsort_cpu.py asserts the edges named here."""
import random

import bammodel

HEAD = "@HD\tVN:1.6\tSO:unsorted\n"
LENGTHS = (37, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 70000)
TIE_GROUPS = (1, 2, 63, 64, 65, 1000)
WINDOW = 4096


def rec(name, ref, pos, flag=0, cigar=(("M", 4),), seq="ACGT", aux=b""):
    return bammodel.bam_record(name, flag, ref, pos, 30, list(cigar), seq, aux=aux)


def unplaced(name, ref=-1, pos=-1):
    return rec(name, ref, pos, flag=4, cigar=())


def file_of(refs, records, head=HEAD, block=600):
    """blocks of `block` inflated bytes: small enough that a segment of a few hundred compressed bytes holds whole ones"""
    text = head + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
    return bammodel.bgzf_compress(bammodel.bam_bytes(text, refs, records), block=block)


def small(raw, parts=6):
    return max(64, len(raw) // parts)


def sized(k, length, ref, pos, flag=0, rng=None):
    """a record of exactly `length` bytes (37 = the 36 fixed bytes and an empty name): a name of up to 20 characters, the rest a Z
    attribute of seeded characters (they deflate to about three quarters, so a long record spans segments)"""
    rng = rng or random.Random(length * 7919 + k)
    extra = length - 37
    n_name = min(extra, 20)
    pad = extra - n_name
    if 0 < pad < 4:                              # the shortest attribute is XZ:Z: with its NUL, four bytes
        n_name, pad = n_name - (4 - pad), 4
    name = (f"{k}." + "n" * 20)[:n_name]
    aux = b"XZZ" + bytes(rng.randrange(48, 112) for _ in range(pad - 4)) + b"\0" if pad else b""
    r = bammodel.bam_record(name, flag, ref, pos, 30, [], "", aux=aux)
    assert len(r) == length, (len(r), length)
    return r


# ---- 1. the hand-built files -------------------------------------------------------------------------------------------------------------
REFS3 = [("chr1", (1 << 31) - 1),("chr2", 1 << 20), ("chr3", 1 << 20)]


def hand():
    R = [rec("c3_500", 2, 500), unplaced("none"), rec("c1_900", 0, 900), rec("c2_rev_700", 1, 700, flag=16), rec("c2_fwd_700", 1, 700),
         unplaced("neg_ref", ref=-7, pos=50), rec("c1_max", 0, (1 << 31) - 1), rec("c1_minus1", 0, -1), rec("c3_fwd_10", 2, 10),
         rec("c3_rev_10", 2, 10, flag=16), rec("c1_flag4", 0, 400, flag=4, cigar=()), rec("c1_100", 0, 100), rec("c2_1", 1, 1),
         rec("c3_500_again", 2, 500)]
    raw = file_of(REFS3, R, block=150)
    return raw, small(raw), 128


HAND_ORDER = ["c1_minus1", "c1_100", "c1_flag4", "c1_900", "c1_max", "c2_1", "c2_fwd_700", "c2_rev_700", "c3_fwd_10", "c3_rev_10", "c3_500",
              "c3_500_again", "none", "neg_ref"]


def header_only():
    return file_of(REFS3, []), 64, WINDOW


def one_record():
    return file_of(REFS3, [rec("only", 1, 5)]), 64, WINDOW


def no_references():
    raw = file_of([], [unplaced(f"u{k}", ref=-1 - (k % 3), pos=(k * 37) % 11 - 1) for k in range(60)], block=200)
    return raw, small(raw), 256


def many_references():
    """3,000 references (the rank takes 12 bits); records on every third one, in an order that is none, and unplaced ones between"""
    refs = [(f"c{r}", 40000) for r in range(3000)]
    rng = random.Random(5)
    R = [rec(f"m{r}_{j}", r, rng.randrange(30000), flag=16 * rng.randrange(2)) for r in range(1, 3000, 3) for j in range(2)] + \
        [rec("last_ref", 2999, 7), rec("first_ref", 0, 7)] + [unplaced(f"u{k}") for k in range(20)]
    rng.shuffle(R)
    raw = file_of(refs, R, block=4000)
    return raw, small(raw), WINDOW


# ---- 2. stability ------------------------------------------------------------------------------------------------------------------------
def ties():
    """tie groups of 1, 2, 63, 64, 65 and 1,000 records: group g lies at (chr1, 1000 * g), forward; the records of all groups interleaved by
    a seeded shuffle, so that every larger group is spread over the file and over its segment borders; names t<group>_<input order>"""
    rng = random.Random(11)
    slots = [g for g, n in enumerate(TIE_GROUPS) for _ in range(n)]
    rng.shuffle(slots)
    seen = [0] * len(TIE_GROUPS)
    R = []
    for g in slots:
        R.append(rec(f"t{g}_{seen[g]}", 0, 1000 * g))
        seen[g] += 1
    raw = file_of([("chr1", 1 << 20)], R, block=3000)
    return raw, small(raw), WINDOW


# ---- 3. the gather -----------------------------------------------------------------------------------------------------------------------
def alignments():
    """3,000 records whose lengths step from 37 bytes up (37 + k mod 48) at seeded positions: in the one-window run the pairs (offset in
    the arena mod 16, offset in the output mod 16) take all 256 values"""
    rng = random.Random(3)
    R = [sized(k, 37 + k % 48, 0, rng.randrange(1 << 20), rng=rng) for k in range(3000)]
    raw = file_of([("chr1", 1 << 20)], R, block=5000)
    return raw, small(raw), WINDOW


def lengths():
    """sorted: 1,023 + 1,025 + 1,024 + 1,024 bytes = one window of exactly WINDOW bytes; then the seven shorter lengths; then the record
    of 70,000 bytes, a window of its own; then 60 records of 900 bytes and more.  The input has them in another order."""
    order = [1023, 1025, 1024, 1024, 37, 63, 64, 65, 255, 256, 257, 70000] + [900 + k for k in range(60)]
    R = [sized(k, n, 0, 100 * (k + 1)) for k, n in enumerate(order)]
    random.Random(17).shuffle(R)
    raw = file_of([("chr1", 1 << 20)], R, block=4000)
    return raw, small(raw, 12), WINDOW


# ---- 4. orders ---------------------------------------------------------------------------------------------------------------------------
def _placed(n, seed):
    rng = random.Random(seed)
    return [rec(f"p{k}", k % 3, 10 * k // 3 + rng.randrange(3), flag=16 * rng.randrange(2), aux=b"XNZ" + b"x" * (k % 23) + b"\0") for k in range(n)]


def already_sorted():
    """sorted input under a header that says so: the product's inflated bytes are the input's"""
    import sortmodel
    _hdr, R = sortmodel.sorted_records(bammodel.bgzf_decompress(file_of(REFS3, _placed(2000, 23))))
    raw = file_of(REFS3, R + [unplaced("u0"), unplaced("u1")], head="@HD\tVN:1.6\tSO:coordinate\n", block=3000)
    return raw, small(raw), WINDOW


def reversed_input():
    """distinct keys in exactly descending order"""
    R = [unplaced("u0")] + [rec(f"r{k}", k % 3, 7 * k, flag=16 * (k & 1)) for k in range(1500)]
    R.sort(key=lambda b: (-(int.from_bytes(b[4:8], "little", signed=True) % 4), -int.from_bytes(b[8:12], "little", signed=True)))
    raw = file_of(REFS3, R, block=3000)
    return raw, small(raw), WINDOW


def seeded(seed=7, n=20000, n_unplaced=300):
    """20,000 records over 5 references and 300 without one, shuffled; runs in segments of 100,000 and of 30,000 bytes, windows of 64 KiB"""
    rng = random.Random(seed)
    refs = [(f"chr{r + 1}", 50_000_000) for r in range(5)]
    R = []
    for k in range(n):
        L = 20 + rng.randrange(60)
        R.append(bammodel.bam_record(f"read{k}", 16 * rng.randrange(2), rng.randrange(5), rng.randrange(40_000_000), 30, [("M", L)], "ACGT" * 3,
                                     aux=b"NMC\x01" + (b"XSZ" + b"s" * rng.randrange(90) + b"\0" if rng.randrange(3) else b"")))
    R += [unplaced(f"unplaced{k}") for k in range(n_unplaced)]
    rng.shuffle(R)
    return file_of(refs, R, block=0xFF00), refs


# ---- 5. the stop -------------------------------------------------------------------------------------------------------------------------
def stop():
    """record 25 has ref_id = n_ref, record 31 a larger one: the first is named -> (raw, segment_bytes, window_bytes, record, read)"""
    R = [rec(f"s{k}", k % 2, 1000 - 10 * k) for k in range(40)]
    R[25] = rec("beyond", 2, 5)
    R[31] = rec("further", 9, 5)
    raw = file_of([("chr1", 1 << 20), ("chr2", 1 << 20)], R, block=300)
    return raw, small(raw), WINDOW, 25, "beyond"


CASES = dict(hand=hand, header_only=header_only, one_record=one_record, no_references=no_references, many_references=many_references, ties=ties,
             alignments=alignments, lengths=lengths, already_sorted=already_sorted, reversed_input=reversed_input)
