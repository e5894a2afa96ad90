"""The inputs of SamView's tests: SAM texts, each with the segment_bytes of its segmented run.  tests/test_samview_cpu.py checks against
tests/sammodel.py that each holds the edges tests/test_samview_gpu.py claims.  Test infrastructure only."""
import numpy as np

import sammodel as sm

REFS = [("chr1", 2 ** 31 - 1), ("chr2", 1_000_000), ("chrM", 16_569)]
HEADER = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in REFS) + "@PG\tID:minimap2\tPN:minimap2\n"
ALPHABET = "=ACMGRSVTWYHKDBN"
SEQ_LENGTHS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 70000]
CIGAR_COUNTS = [0, 1, 63, 64, 65, 200, 65535]
ATTR_COUNTS = [0, 1, 63, 64, 65, 130]
INT_EDGES = [-2 ** 31, -32769, -32768, -129, -128, 127, 128, 255, 256, 32767, 32768, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
FLOATS = ["0", "-0.0", "+1.5", "3.1416", "0.0001", "-12345.6789", "1e5", "1E-5", "2.5e+10", "123456789012345", "0.000123456789012345",
          "999999999999999e22", "1e-22", "1.", ".5", "1.e2", "0.1", "16777217", "inf", "-inf", "nan"]
BAD_FLOATS = ["1234567890123456", "1e23", "1e-23", "0.1e-22", "+inf", "Inf", "NaN", "infinity", "1e", "e5", ".", "", "1.2.3", "0x10", "1e12345", "1 "]
B_COUNTS = [0, 1, 64, 65]
B_VALUES = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}


def line(name="r", flag=0, rname="chr1", pos=100, mapq=60, cigar="*", rnext="*", pnext=0, tlen=0, seq="*", qual="*", attrs=()):
    return "\t".join([name, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), seq, qual, *attrs])


def text(lines, header=HEADER, last_lf=True):
    body = "\n".join(lines) + ("\n" if lines and last_lf else "")
    return (header + body).encode("latin-1")


def bases(rng, n):
    """n bases over the alphabet in either case, with a byte outside it now and then"""
    pool = np.frombuffer((ALPHABET + ALPHABET.lower() + "xz!.").encode(), dtype=np.uint8)
    return rng.choice(pool, n).tobytes().decode("latin-1")


def quals(rng, n):
    return (rng.integers(33, 127, n, dtype=np.uint8)).tobytes().decode("latin-1")


def hand():
    """a handful of ordinary lines: a mapped read with attributes, its secondary without sequence, an unmapped read, a mate pair"""
    ls = [line("read/1", 0, "chr1", 1001, 60, "5S20M2I10M3D8M1000N5M", "*", 0, 0, "ACGTN" * 10, "I" * 50, ("NM:i:3", "ms:i:40", "tp:A:P", "de:f:0.0123", "SA:Z:chr2,5,+,10M,60,0;")),
          line("read/1", 256, "chr2", 5, 0, "10M", "*", 0, 0, "*", "*", ("NM:i:0",)),
          line("unmapped", 4, "*", 0, 0, "*", "*", 0, 0, "acgtn", "*"),
          line("pair", 99, "chr1", 7, 30, "4M", "=", 107, 104, "ACGT", "!~IJ", ("XB:B:c,-1,2", "XH:H:1AE3")),
          line("pair", 147, "chr1", 107, 30, "4M", "chrM", 7, -104, "ACGT", "*")]
    return text(ls), 3


def seq_lengths():
    """every SEQ length of SEQ_LENGTHS with QUAL * and with QUAL; the names of 1 .. 4 bytes put the records at every offset mod 4"""
    rng = np.random.default_rng(11)
    ls = []
    for k, n in enumerate(SEQ_LENGTHS):
        for with_qual in (False, True):
            seq = bases(rng, n) if n else "*"
            ls.append(line("n" * (1 + len(ls) % 4), 0, "chr2", 1 + k, 20, f"{n}M" if n else "*", seq=seq, qual=quals(rng, n) if with_qual and n else "*",
                           attrs=("NM:i:1",) if k % 2 else ()))
    ls.append(line("lower", 0, "chr1", 1, 0, "*", seq="acgt=ACGT", qual="*"))
    ls.append(line("outside", 0, "chr1", 1, 0, "*", seq="A.C\x80G\xffT@[`{", qual="!" * 11))
    return text(ls), 4096


def cigars():
    """CIGAR * and 1 .. 65,535 operations, every letter, the lengths 1 and 2^28 - 1, and CIGARs of reference length 0"""
    ls = [line(f"c{n}", 0, "chr1", 10 + n, 1, "".join(f"{1 + k % 9}{'MIDNSHP=X'[k % 9]}" for k in range(n)) or "*") for n in CIGAR_COUNTS]
    ls.append(line("letters", 0, "chr1", 1, 0, "1M1I1D1N1S1H1P1=1X"))
    ls.append(line("longest", 0, "chr1", 1, 0, f"{2 ** 28 - 1}M{2 ** 28 - 1}D1M"))
    ls.append(line("zeros", 0, "chr1", 1, 0, "007M0I"))
    ls.append(line("clip", 0, "chr1", 16384, 0, "5S", seq="ACGTA"))
    ls.append(line("insert", 0, "chr1", 16384, 0, "3I2S", seq="ACGTA"))
    return text(ls), 600


def b_values(st, n):
    if st == "f":
        return [FLOATS[k % len(FLOATS)] for k in range(n)]
    lo, hi = B_VALUES[st]
    return [str([lo, hi, 0, 1][k % 4]) for k in range(n)]


def attributes():
    """0 .. 130 attributes on a line, every type, i on both sides of every border of int_type, the float texts, B of every subtype with
    0, 1, 64 and 65 values, Z values of 0, 1 and 5,000 bytes"""
    ls = [line(f"a{n}", 0, "chr1", 1, 0, "*", attrs=[f"X{chr(65 + k // 26)}:i:{k * 977 - 60000}" if k % 3 else f"Y{chr(65 + k // 26)}:Z:v{k}" for k in range(n)])
          for n in ATTR_COUNTS]
    ls.append(line("types", 0, "chr1", 1, 0, "*", attrs=["XA:A:!", "XB:A:~", "XI:i:-7", "XP:i:+7", "XF:f:1.25", "XZ:Z:a b:c", "XH:H:00ff1A", "XE:H:", "XX:B:c,1"]))
    ls.append(line("ints", 0, "chr1", 1, 0, "*", attrs=[f"I{chr(65 + k)}:i:{v}" for k, v in enumerate(INT_EDGES)]))
    ls.append(line("floats", 0, "chr1", 1, 0, "*", attrs=[f"F{chr(65 + k)}:f:{v}" for k, v in enumerate(FLOATS)]))
    for st in "cCsSiIf":
        ls.append(line(f"B{st}", 0, "chr1", 1, 0, "*", attrs=[f"B{k}:B:{st}" + "".join("," + v for v in b_values(st, n)) for k, n in enumerate(B_COUNTS)]))
    ls.append(line("z", 0, "chr1", 1, 0, "*", seq="ACGT", qual="IIII", attrs=["Z0:Z:", "Z1:Z:x", "Z2:Z:" + "long value " * 454 + "123456", "NM:i:0"]))
    return text(ls), 2048


N_MANY = 3000
MANY_HEADER = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:contig_{k}\tLN:{2 ** 31 - 1 if k == 7 else 1000 + k}\tM5:x\n" for k in range(N_MANY))


def names_and_positions():
    """names of 1 and 254 bytes, the first and the last of 3,000 references, RNEXT = * and a name, POS 0 and 2^31 - 1, bin on both
    sides of a 16 kb, a 128 kb and a 512 Mb border"""
    big = "contig_7"
    ls = [line("a", 0, "contig_0", 5, 0, "3M", "=", 9, 7),
          line("b" * 254, 16, f"contig_{N_MANY - 1}", 1, 255, "1M", "contig_0", 2 ** 31 - 1, -2 ** 31),
          line("unplaced", 0, "*", 0, 0, "*", "*", 0, 2 ** 31 - 1),
          line("on_ref_pos0", 4, big, 0, 0, "*", f"contig_{N_MANY - 1}", 0, 0),
          line("last_pos", 0, big, 2 ** 31 - 1, 0, "1M"),
          line("last_pos_long", 0, big, 2 ** 31 - 1, 0, f"{2 ** 28 - 1}M"),
          line("in16k", 0, big, 16384, 0, "1M"), line("over16k", 0, big, 16384, 0, "2M"), line("next16k", 0, big, 16385, 0, "1M"),
          line("in128k", 0, big, 131072, 0, "1M"), line("over128k", 0, big, 131072, 0, "2M"), line("next128k", 0, big, 131073, 0, "1M"),
          line("in512m", 0, big, 2 ** 29, 0, "1M"), line("over512m", 0, big, 2 ** 29, 0, "2M"), line("next512m", 0, big, 2 ** 29 + 1, 0, "1M"),
          line("whole", 0, big, 1, 0, f"{2 ** 28 - 1}N" * 7)]
    return text(ls, MANY_HEADER), 700


def header_only():
    return HEADER.encode(), 16


def header_only_open():
    return HEADER.encode()[:-1], 16


def empty():
    return b"", 16


def no_header():
    return text([line("u1", 4, "*", 0, 0, "*", seq="ACGT", qual="IIII"), line("u2", 4, "*", 0, 0, "*", "*", 0, 0, "AC", "*", ("RG:Z:x",))], header=""), 9


def last_line_open():
    raw, seg = hand()
    return raw[:-1], seg


def long_header():
    """a header several segments long"""
    return text([line("r", 0, "contig_2999", 3, 0, "2M")], MANY_HEADER), 500


CASES = dict(hand=hand, seq_lengths=seq_lengths, cigars=cigars, attributes=attributes, names_and_positions=names_and_positions, header_only=header_only,
             header_only_open=header_only_open, empty=empty, no_header=no_header, last_line_open=last_line_open, long_header=long_header)

GOOD = line("good", 0, "chr1", 1, 0, "1M", seq="A", qual="I")


def stops():
    """name -> (the text, the 1-based line of the stop, its rule in sammodel.REASONS): one bad line behind two good ones"""
    def one(bad, header=HEADER):
        return text([GOOD, GOOD, bad, GOOD], header), header.count("\n") + 3

    out = {}

    def add(name, bad, rule, header=HEADER):
        raw, at = one(bad, header)
        out[name] = (raw, at, sm.REASONS[rule])

    add("late_header", "@CO\tlate", sm.LATE)
    add("ten_fields", "\t".join(GOOD.split("\t")[:10]), sm.FIELDS)
    add("blank_line", "", sm.FIELDS)
    add("name_255", line("n" * 255), sm.NAME)
    add("name_empty", line(""), sm.NAME)
    add("flag_65536", line(flag=65536), sm.FLAG)
    add("flag_text", line(flag="0x4"), sm.FLAG)
    add("unknown_rname", line(rname="chr3"), sm.RNAME)
    out["rname_without_header"] = (text([line(rname="*"), line(rname="chr1")], ""), 2, sm.REASONS[sm.RNAME])
    add("rname_equals", line(rname="="), sm.RNAME)
    add("pos_2_31", line(pos=2 ** 31), sm.POS)
    add("pos_negative", line(pos=-1), sm.POS)
    add("mapq_256", line(mapq=256), sm.MAPQ)
    add("cigar_2_28", line(cigar=f"{2 ** 28}M"), sm.CIGAR)
    add("cigar_letter", line(cigar="5M3Q"), sm.CIGAR)
    add("cigar_no_length", line(cigar="M"), sm.CIGAR)
    add("cigar_trailing_digits", line(cigar="5M3"), sm.CIGAR)
    add("cigar_empty", line(cigar=""), sm.CIGAR)
    add("cigar_65536", line(cigar="1M1I" * 32768), sm.CIGAR_MANY)
    add("unknown_rnext", line(rnext="chrX"), sm.RNEXT)
    add("pnext_2_31", line(pnext=2 ** 31), sm.PNEXT)
    add("tlen_2_31", line(tlen=2 ** 31), sm.TLEN)
    add("tlen_below", line(tlen=-2 ** 31 - 1), sm.TLEN)
    add("qual_short", line(seq="ACGT", qual="III"), sm.QUAL_LEN)
    add("qual_without_seq", line(seq="*", qual="II"), sm.QUAL_LEN)
    add("attr_short", line(attrs=["NM:i"]), sm.ATTR)
    add("attr_type", line(attrs=["NM:x:1"]), sm.ATTR)
    add("attr_A_two", line(attrs=["XA:A:ab"]), sm.ATTR)
    add("attr_empty", line(attrs=["", "NM:i:1"]), sm.ATTR)
    add("int_2_32", line(attrs=["NM:i:1", f"XI:i:{2 ** 32}"]), sm.ATTR_INT)
    add("int_below", line(attrs=[f"XI:i:{-2 ** 31 - 1}"]), sm.ATTR_INT)
    add("int_text", line(attrs=["XI:i:1.0"]), sm.ATTR_INT)
    for k, v in enumerate(BAD_FLOATS):
        add(f"float_{k}", line(attrs=[f"XF:f:{v}"]), sm.ATTR_FLOAT)
    add("B_subtype", line(attrs=["XB:B:d,1"]), sm.ATTR_B)
    add("B_none", line(attrs=["XB:B:"]), sm.ATTR_B)
    add("B_range", line(attrs=["XB:B:C,255,256"]), sm.ATTR_B)
    add("B_empty_value", line(attrs=["XB:B:s,"]), sm.ATTR_B)
    add("B_no_comma", line(attrs=["XB:B:s1"]), sm.ATTR_B)
    add("B_float", line(attrs=["XB:B:f,1.5,1e23"]), sm.ATTR_B)
    out["sq_without_ln"] = (text([GOOD], "@HD\tVN:1.6\n@SQ\tSN:chr1\n"), 2, sm.SQ_REASON)
    out["sq_without_sn"] = (text([GOOD], "@SQ\tSN:chr1\tLN:5\n@SQ\tLN:10\n"), 2, sm.SQ_REASON)
    return out


def two_bad_lines():
    """two bad lines in one segment: the first one is named -> (text, line, reason)"""
    ls = [GOOD] * 40 + [line(mapq=999)] + [GOOD] * 3 + [line(flag=-1)] + [GOOD] * 5
    return text(ls), HEADER.count("\n") + 41, sm.REASONS[sm.MAPQ]


def late_stop():
    """a stop in a later segment (segment_bytes 2,000 against about 30 bytes a line) -> (text, segment_bytes, line, reason)"""
    ls = [GOOD] * 500 + [line(seq="ACGT", qual="II")] + [GOOD] * 10
    return text(ls), 2000, HEADER.count("\n") + 501, sm.REASONS[sm.QUAL_LEN]


SEEDED_LINES = 20_000


def seeded(n=SEEDED_LINES, seed=3, ordered=False):
    """n lines of a long-read pipeline's mix: primary records with SEQ and QUAL of 50 .. 900 bases and minimap2's attributes, and
    secondary records without sequence; ordered: by reference and position, as a sorted file has them"""
    rng = np.random.default_rng(seed)
    where = sorted((int(rng.integers(0, 3)), int(rng.integers(1, 16_000))) for _ in range(n)) if ordered else None
    ls = []
    for k in range(n):
        ref, pos = where[k] if ordered else (int(rng.integers(0, 3)), int(rng.integers(1, 16_000)))
        primary = rng.random() < 0.7
        m = int(rng.integers(50, 900))
        cigar = f"{int(rng.integers(0, 40))}S{m}M{int(rng.integers(1, 30))}D{int(rng.integers(1, 200))}M{int(rng.integers(50, 3000))}N{int(rng.integers(1, 90))}M"
        attrs = [f"NM:i:{int(rng.integers(0, 70000))}", f"ms:i:{int(rng.integers(-200, 400))}", "tp:A:" + "PS"[int(rng.integers(0, 2))],
                 f"de:f:{rng.integers(0, 10000) / 10000:.4f}", f"BC:Z:{bases(rng, 16)}", f"U8:Z:{bases(rng, 12)}"]
        if primary:
            n_b = m + int(rng.integers(0, 300))
            ls.append(line(f"read_{k}", 16 * int(rng.integers(0, 2)), REFS[ref][0], pos, int(rng.integers(0, 61)), cigar, seq=bases(rng, n_b), qual=quals(rng, n_b),
                           attrs=attrs))
        else:
            ls.append(line(f"read_{k}", 256, REFS[ref][0], pos, 0, cigar, attrs=attrs[:3]))
    return text(ls)
