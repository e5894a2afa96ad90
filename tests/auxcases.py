"""The attribute-size rule of csrc/smi_longread.h (lr::aux_size), the one gate for attribute bytes from outside on the host and in the
kernels that walk attributes: a plain model of the SAM specification's rule (section 4.2.4: tag, type, value; Z and H end with a NUL;
B holds an element type, a 32-bit count and count elements) and the smallest attribute lists that can go wrong."""
import struct

FINE, TRUNCATED, SHORT_ARRAY, BAD_ELEMENT, BAD_TYPE = range(5)  # lr::AuxBad
WIDTH = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
ELEMENT = {t: w for t, w in WIDTH.items() if t != "A"}


def size(blob, p):
    """(bytes of the attribute at blob[p:], FINE) or (0, why it is refused); nothing behind the list counts"""
    left = len(blob) - p
    if left < 3:
        return 0, TRUNCATED
    t = chr(blob[p + 2])
    if t in WIDTH:
        n = 3 + WIDTH[t]
    elif t in "ZH":
        z = blob.find(b"\0", p + 3)
        if z < 0:
            return 0, TRUNCATED
        n = z + 1 - p
    elif t == "B":
        if left < 8:
            return 0, SHORT_ARRAY
        e = chr(blob[p + 3])
        if e not in ELEMENT:
            return 0, BAD_ELEMENT
        n = 8 + ELEMENT[e] * struct.unpack_from("<I", blob, p + 4)[0]
    else:
        return 0, BAD_TYPE
    return (n, FINE) if n <= left else (0, TRUNCATED)


def walk(blob):
    """the steps of a reader from the first byte: every attribute's size, and the refusal it stops at"""
    steps, p = [], 0
    while p < len(blob):
        n, why = size(blob, p)
        steps.append((n, why))
        if why:
            break
        p += n
    return steps


def _scalar(t, tag=b"XS"):
    return tag + t.encode() + bytes(range(1, 1 + WIDTH[t]))


def _array(e, count, payload=None, tag=b"XB"):
    body = bytes(ELEMENT.get(e, 1) * count) if payload is None else payload
    return tag + b"B" + e.encode() + struct.pack("<I", count) + body


GOOD = b"NHC\x01"  # an attribute in front, so that the walk has taken a step before it meets the case

CASES = {"empty": b"", "one_byte": b"X", "two_bytes": b"XY", "tag_and_type": b"XYi", "good_then_one": GOOD + b"X", "good_then_two": GOOD + b"XY",
         "z": GOOD + b"XZZabc\0", "z_empty": b"XZZ\0", "z_no_nul": GOOD + b"XZZabc", "z_no_value": b"XZZ", "z_then_good": b"XZZab\0" + GOOD,
         "h": GOOD + b"XHH1aF0\0", "h_odd": b"XHH1aF\0" + GOOD, "h_not_hex": b"XHHxy\0", "h_no_nul": GOOD + b"XHH1a", "h_empty": b"XHH\0",
         "b_seven_left": GOOD + b"XBBc\0\0\0", "b_header_only_type": b"XBB", "b_bad_element": GOOD + _array("A", 1),
         "b_bad_element_short": b"XBBZ\0\0\0",  # (fewer than 8 bytes: the header's rule comes first)
         "b_one_past": GOOD + _array("s", 3)[:-1], "b_one_past_i": _array("i", 1)[:-1], "b_huge": GOOD + _array("c", 0xffffffff, b"\1\2\3"),
         "b_huge_f": _array("f", 0xffffffff, b""), "b_then_good": _array("S", 2) + GOOD,
         "bad_type": GOOD + b"XYz\0\0\0\0", "bad_type_nul": b"XY\0\0", "bad_type_last": GOOD + b"XYq"}
for _t in WIDTH:
    CASES[f"scalar_{_t}"] = GOOD + _scalar(_t)
    CASES[f"scalar_{_t}_short"] = GOOD + _scalar(_t)[:-1]
for _e in ELEMENT:
    CASES[f"b_{_e}_0"] = GOOD + _array(_e, 0) + GOOD
    CASES[f"b_{_e}_1"] = _array(_e, 1) + GOOD

# attribute bytes behind a record's own attributes, one list per way of going wrong: every program that walks a record's attributes, on the
# host or in a kernel, refuses the record (tests/longreadcases.py, moltagcases.py and fusionprepcases.py hand them to their programs)
DAMAGED = {k: CASES[k] for k in ("good_then_one", "good_then_two", "scalar_i_short", "scalar_A_short", "z_no_nul", "h_no_nul", "b_seven_left",
                                 "b_bad_element", "b_one_past", "b_huge", "bad_type")}
