"""SamView's definition in plain Python: SAM text -> the BAM header's bytes and the records' bytes, or the stop
with its 1-based line and its reason.  Also the way back, a BAM record of bammodel.parse_bam as a SAM line.  Test infrastructure only."""
import re
import struct

from bammodel import CIGAR_OPS, reg2bin

SEQ_CODE = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}

BASE_CODES = bytes(SEQ_CODE.get(chr(c).upper(), 15) if c < 128 else 15 for c in range(256))
MINUS_33 = bytes((c - 33) & 255 for c in range(256))

# the rules in the order a line that breaks several of them is named with
REASONS = [
    "a header line behind the first alignment line",
    "fewer than 11 fields",
    "the read name is empty or longer than 254 bytes",
    "FLAG is not a number in 0 .. 65535",
    "RNAME is not * or one of the header's references",
    "POS is not a number in 0 .. 2^31 - 1",
    "MAPQ is not a number in 0 .. 255",
    "CIGAR is not * or operations of MIDNSHP=X with lengths of 1 .. 9 digits below 2^28",
    "CIGAR has more than 65535 operations (the CG form is not built)",
    "RNEXT is not *, = or one of the header's references",
    "PNEXT is not a number in 0 .. 2^31 - 1",
    "TLEN is not a number in -2^31 .. 2^31 - 1",
    "QUAL and SEQ differ in length",
    "an attribute is not TAG:TYPE:VALUE with a type of AifZHB",
    "an i attribute is not a number in -2^31 .. 2^32 - 1",
    "an f attribute is not inf, -inf, nan or a decimal of at most 15 significant digits and a power of ten within 22",
    "a B attribute has no subtype of cCsSiIf or a value outside its subtype",
]
(LATE, FIELDS, NAME, FLAG, RNAME, POS, MAPQ, CIGAR, CIGAR_MANY, RNEXT, PNEXT, TLEN, QUAL_LEN, ATTR, ATTR_INT, ATTR_FLOAT, ATTR_B) = range(17)
SQ_REASON = "an @SQ line without SN or an LN in 0 .. 2^31 - 1"

UNSIGNED = re.compile(rb"[0-9]{1,10}\Z")
SIGNED = re.compile(rb"[-+]?[0-9]{1,10}\Z")
FLOAT = re.compile(rb"[-+]?(?=[0-9]|\.[0-9])([0-9]*)(?:\.([0-9]*))?(?:[eE]([-+]?[0-9]{1,4}))?\Z")
CIGAR_OP = re.compile(rb"([0-9]*)([^0-9])")
RANGES = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}
PACK = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


class Stop(Exception):
    def __init__(self, line, reason):
        super().__init__(f"line {line}: {reason}")
        self.line, self.reason = line, reason


def int_type(v):
    """htsjdk's getIntegerType: the first of c C s S i I that holds v"""
    return next(t for t in "cCsSiI" if RANGES[t][0] <= v <= RANGES[t][1])


def float_bits(text):
    """the four bytes of an f value, or None outside the class: inf, -inf, nan, or sign, at most 15 significant digits with an optional
    fraction, an optional exponent, the power of ten left when the digits are read as an integer within +-22"""
    if text in (b"inf", b"-inf", b"nan"):
        return struct.pack("<f", float(text))
    m = FLOAT.match(text)
    if not m:
        return None
    whole, frac, ex = m.group(1), m.group(2) or b"", int(m.group(3) or 0)
    if len((whole + frac).lstrip(b"0")) > 15 or not -22 <= ex - len(frac) <= 22:
        return None
    return struct.pack("<f", float(text))


def attribute(a):
    """one TAG:TYPE:VALUE -> its bytes in the record, or the number of the rule it breaks"""
    if len(a) < 5 or a[2:3] != b":" or a[4:5] != b":":
        return ATTR
    tag, ty, v = a[:2], chr(a[3]), a[5:]
    if ty == "A":
        return tag + b"A" + v if len(v) == 1 else ATTR
    if ty == "i":
        if not SIGNED.match(v) or not -2 ** 31 <= int(v) <= 2 ** 32 - 1:
            return ATTR_INT
        t = int_type(int(v))
        return tag + t.encode() + struct.pack(PACK[t], int(v))
    if ty == "f":
        bits = float_bits(v)
        return ATTR_FLOAT if bits is None else tag + b"f" + bits
    if ty in "ZH":
        return tag + ty.encode() + v + b"\0"
    if ty == "B":
        st = chr(v[0]) if v else ""
        if st not in list("cCsSiIf"):
            return ATTR_B
        if len(v) > 1 and v[1:2] != b",":
            return ATTR_B
        vals = v[2:].split(b",") if len(v) > 1 else []
        out = []
        for x in vals:
            if st == "f":
                bits = float_bits(x)
                if bits is None:
                    return ATTR_B
                out.append(bits)
            else:
                if not SIGNED.match(x) or not RANGES[st][0] <= int(x) <= RANGES[st][1]:
                    return ATTR_B
                out.append(struct.pack(PACK[st], int(x)))
        return tag + b"B" + st.encode() + struct.pack("<I", len(out)) + b"".join(out)
    return ATTR


def record(line, refs):
    """one alignment line (without its LF) -> the record's bytes, or the number of the first rule it breaks"""
    bad = set()
    if line[:1] == b"@":
        bad.add(LATE)
    f = line.split(b"\t")
    if len(f) < 11:
        bad.add(FIELDS)
    if bad:
        return min(bad)
    name, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]

    def number(text, rule, hi, signed=False):
        if not (SIGNED if signed else UNSIGNED).match(text) or not (-hi - 1 if signed else 0) <= int(text) <= hi:
            bad.add(rule)
            return 0
        return int(text)

    def ref(text, rule, same=None):
        if text == b"*":
            return -1
        if same is not None and text == b"=":
            return same
        if text not in refs:
            bad.add(rule)
            return -1
        return refs[text]

    if not 1 <= len(name) <= 254:
        bad.add(NAME)
    flag = number(flag, FLAG, 65535)
    ref_id = ref(rname, RNAME)
    pos = number(pos, POS, 2 ** 31 - 1) - 1
    mapq = number(mapq, MAPQ, 255)
    next_ref = ref(rnext, RNEXT, ref_id)
    next_pos = number(pnext, PNEXT, 2 ** 31 - 1) - 1
    tlen = number(tlen, TLEN, 2 ** 31 - 1, signed=True)
    ops, ref_len = [], 0
    if cigar != b"*":
        at = 0
        for m in CIGAR_OP.finditer(cigar):
            digits, op = m.group(1), m.group(2).decode("latin-1")
            if m.start() != at or op not in CIGAR_OPS or not 1 <= len(digits) <= 9 or int(digits) >= 2 ** 28:
                bad.add(CIGAR)
                break
            at = m.end()
            ops.append(int(digits) << 4 | CIGAR_OPS.index(op))
            if op in "MDN=X":
                ref_len += int(digits)
        if not cigar or at != len(cigar):
            bad.add(CIGAR)
        if len(CIGAR_OP.findall(cigar)) > 65535:
            bad.add(CIGAR_MANY)
    l_seq = 0 if seq == b"*" else len(seq)
    if qual != b"*" and len(qual) != l_seq:
        bad.add(QUAL_LEN)
    aux = []
    for a in f[11:]:
        b = attribute(a)
        if isinstance(b, int):
            bad.add(b)
        else:
            aux.append(b)
    if bad:
        return min(bad)
    codes = seq[:l_seq].translate(BASE_CODES) + b"\0"           # either case; a byte outside the alphabet is N
    packed = bytes(a << 4 | b for a, b in zip(codes[0:l_seq:2], codes[1::2]))
    q = b"\xff" * l_seq if qual == b"*" else qual.translate(MINUS_33)
    bin_ = 4680 if pos < 0 else reg2bin(pos, pos + (ref_len or 1)) & 0xFFFF
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) + 1, mapq, bin_, len(ops), flag, l_seq, next_ref, next_pos, tlen)
    body += name + b"\0" + struct.pack(f"<{len(ops)}I", *ops) + bytes(packed) + q + b"".join(aux)
    return struct.pack("<I", len(body)) + body


def split_header(text):
    """-> (the leading @ lines as they stand, the rest, the number of header lines)"""
    at = n = 0
    while text[at:at + 1] == b"@":
        nl = text.find(b"\n", at)
        at = len(text) if nl < 0 else nl + 1
        n += 1
    return text[:at], text[at:], n


def bam_header(header_text):
    """-> (the BAM header's bytes, {reference name: its number})"""
    refs, entries = {}, []
    for k, ln in enumerate(header_text.split(b"\n")):
        f = ln.split(b"\t")
        if f[0] != b"@SQ":
            continue
        sn = [x[3:] for x in f if x[:3] == b"SN:"]
        ln_ = [int(x[3:]) for x in f if x[:3] == b"LN:" and UNSIGNED.match(x[3:]) and int(x[3:]) <= 2 ** 31 - 1]
        if not sn or not sn[0] or not ln_:
            raise Stop(k + 1, SQ_REASON)
        refs.setdefault(sn[0], len(entries))
        entries.append(struct.pack("<I", len(sn[0]) + 1) + sn[0] + b"\0" + struct.pack("<I", ln_[0]))
    return b"BAM\1" + struct.pack("<I", len(header_text)) + header_text + struct.pack("<I", len(entries)) + b"".join(entries), refs


def convert(text):
    """SAM text -> (the BAM header's bytes, the records' bytes one by one); Stop at the first line that breaks a rule"""
    header_text, body, n_header = split_header(text)
    header, refs = bam_header(header_text)
    lines = body.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    out = []
    for k, ln in enumerate(lines):
        r = record(ln, refs)
        if isinstance(r, int):
            raise Stop(n_header + k + 1, REASONS[r])
        out.append(r)
    return header, out


def stream(text):
    header, recs = convert(text)
    return header + b"".join(recs)


def aux_text(aux):
    """the attribute bytes of a BAM record as TAG:TYPE:VALUE fields (integers come back as i, which SamView gives its type again)"""
    out, p = [], 0
    while p < len(aux):
        tag, ty = aux[p:p + 2].decode(), chr(aux[p + 2])
        p += 3
        if ty == "A":
            out.append(f"{tag}:A:{chr(aux[p])}")
            p += 1
        elif ty in PACK:
            n = struct.calcsize(PACK[ty])
            out.append(f"{tag}:i:{struct.unpack_from(PACK[ty], aux, p)[0]}")
            p += n
        elif ty in "ZH":
            e = aux.index(b"\0", p)
            out.append(f"{tag}:{ty}:{aux[p:e].decode('latin-1')}")
            p = e + 1
        elif ty == "f":
            out.append(f"{tag}:f:{struct.unpack_from('<f', aux, p)[0]!r}")
            p += 4
        else:
            st, n = chr(aux[p]), struct.unpack_from("<I", aux, p + 1)[0]
            fmt = "<f" if st == "f" else PACK[st]
            vals = [struct.unpack_from(fmt, aux, p + 5 + k * struct.calcsize(fmt))[0] for k in range(n)]
            out.append(f"{tag}:B:{st}" + "".join(f",{v!r}" for v in vals))
            p += 5 + n * struct.calcsize(fmt)
    return out


def sam_line(r, refs):
    """a record of bammodel.parse_bam -> its SAM line (mate fields * 0 0, as bammodel.bam_record leaves them)"""
    cigar = "".join(f"{n}{op}" for op, n in r["cigar"]) or "*"
    qual = "*" if r["qual"] == b"\xff" * len(r["qual"]) else bytes(q + 33 for q in r["qual"]).decode("latin-1")
    f = [r["name"], str(r["flag"]), refs[r["ref_id"]][0] if r["ref_id"] >= 0 else "*", str(r["pos0"] + 1), str(r["mapq"]), cigar, "*", "0", "0",
         r["seq"] or "*", qual if r["seq"] else "*"] + aux_text(r["aux"])
    return "\t".join(f).encode("latin-1")


def sam_text(header_text, refs, recs):
    return header_text.encode() + b"".join(sam_line(r, refs) + b"\n" for r in recs)
