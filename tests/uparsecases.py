"""Chunks for K-UPARSE (k_umi_parse of smi_umi_stage.hip) at its edges: marker and tag layouts, number forms, Q forms, UMI window limits, every
return of the CIGAR walk, names longer than the LDS stage, partial waves, grouping keys, and the names that must hand the chunk to the host
path.  Test infrastructure only; everything is built from literals and seeds.  Every case is a function returning
(names, flags, pos0, cigars, kwargs) for Context.assignumis_chunk; tests/uparsemodel.py says what the chunk owes."""
import re

import numpy as np

NAME_STAGE = 320                                   # kNameStage of smi_umi_stage.hip (tests/test_uparse_cases_cpu.py compares)
FLAT_LIMIT = 64 * (NAME_STAGE + 4) - 16            # a wave whose 64 names hold more bytes than this stages row by row (the `!flat` branch)
BC0 = "ACGTACGTACGTACGT"
OPS = "MIDNSHP=X"
_DEC = {1: "A", 2: "G", 4: "C", 8: "T", 15: "N"}
_COMP = {1: "T", 2: "C", 4: "G", 8: "A", 15: "N"}  # the letter whose complement has code c
X_LEN, POS = 43, 19                                # X= of 43 bases, barcode end at 19 on the strand the window is read from
QS = ["12", "15.5", "9.25", "20.125", "7", "18.75", "11"]
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


# ---- the forms K-UPARSE evaluates itself ---------------------------------------------------------------------------------------------------
def _value(sub, tag):
    i = sub.find(tag)
    if i < 0:
        return None
    i += len(tag)
    j = sub.find("_", i)
    return sub[i:] if j < 0 else sub[i:j]


def _int_form(v, must_be_number=False):
    """digits with an optional '-', at most 10 of them, inside int; or (where the field may be absent) text that no parser takes for a number:
    its first character that is no digit is neither a blank nor a '+'"""
    if v == "":
        return not must_be_number
    body = v[1:] if v[0] == "-" else v
    if not 1 <= len(body) <= 10:
        return False
    if body.isdigit():
        return INT_MIN <= int(v) <= INT_MAX
    if must_be_number:
        return False
    first = next(c for c in body if not c.isdigit())
    return first not in " +\t"


def evaluated_on_device(name):
    """the rule of K-UPARSE: a name it evaluates itself has AE= as a number behind its marker, PS= / ed= / bcEnd= as numbers (or as text no
    parser reads as one), a bc= of 16 letters ACGT, and a Q= of at most 7 digits, at most 3 of them decimals.  Anything else sends the whole
    chunk to the host path.  (A name without a marker carries nothing to evaluate.)"""
    k = name.find("_REV_")
    if k < 0:
        k = name.find("_FWD_")
    if k < 0:
        return True
    sub = name[k + 4:]
    ae = _value(sub, "AE=")
    if ae is None or not _int_form(ae, must_be_number=True):
        return False
    for tag in ("PS=", "ed=", "bcEnd="):
        v = _value(sub, tag)
        if v is not None and not _int_form(v):
            return False
    bc = _value(sub, "bc=")
    if bc is not None and not re.fullmatch("[ACGT]{16}", bc):
        return False
    q = _value(sub, "Q=")
    if q is not None:
        m = re.fullmatch(r"([0-9]*)(?:\.([0-9]*))?", q)
        if not m or not 1 <= len(m.group(1)) + len(m.group(2) or "") <= 7 or len(m.group(2) or "") > 3:
            return False
    return True


# ---- building blocks -----------------------------------------------------------------------------------------------------------------------
def window_x(w, five, pos=POS, x_len=X_LEN, fill="A"):
    """an X= value whose UMI window (barcode end `pos`) holds the codes of w: 5' on X= itself, 3' on its reverse complement"""
    x = [fill] * x_len
    for k, c in enumerate(w):
        i = pos - 1 + k if five else x_len - (pos + k)
        if 0 <= i < x_len:                             # (a window that does not fit is cut off: such a read has none)
            x[i] = _DEC[int(c)] if five else _COMP[int(c)]
    return "".join(x)


def fields(w, q="15", five=False, bc=BC0, **over):
    """the tags of a pass-2 name in scanfastq's order, as a list of (tag, text); over: other texts for some tags (None drops the tag)"""
    if five:
        f = [("AE", "50"), ("bc", bc), ("ed", "0"), ("bcStart", "51"), ("bcEnd", "66"), ("X", window_x(w, True)), ("Q", q)]
    else:
        f = [("PS", "700"), ("PE", "730"), ("AE", "743"), ("bc", bc), ("ed", "0"), ("ed_sec", "3"), ("bcStart", "742"), ("bcEnd", "727"),
             ("X", window_x(w, False)), ("Q", q)]
    for k, v in over.items():
        assert any(t == k for t, _ in f), k
    return [(t, over.get(t, v)) for t, v in f if over.get(t, v) is not None]


def join(rid, f, marker="_FWD_", tail="1a"):
    return rid + marker + "_".join(f"{t}={v}" for t, v in f) + ("" if tail is None else "_" + tail)


def row(name, pos0=100_000, flag=0, cigar=(("M", 1000),)):
    return dict(name=name, pos0=pos0, flag=flag, cigar=list(cigar))


def finish(rows, **kw):
    names = [r["name"] for r in rows]
    flags = np.array([r["flag"] for r in rows], dtype=np.uint16)
    pos0 = np.array([r["pos0"] for r in rows], dtype=np.int32)
    cigars = [np.array([(ln << 4) | OPS.index(op) for op, ln in r["cigar"]], dtype=np.uint32) for r in rows]
    return names, flags, pos0, cigars, kw


def umis(rng, n, ul=12):
    return rng.choice([1, 2, 4, 8], size=(n, ul + 2)).astype(np.uint8)


def near(w, p, shift=1):
    """w with the base at p replaced by another one: UMI distance 1"""
    o = np.array(w, dtype=np.uint8).copy()
    o[p] = [1, 2, 4, 8][([1, 2, 4, 8].index(int(o[p])) + shift) % 4]
    return o


def barcode(rng):
    return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 16))


def pad_window(w, ul):
    """the standard names hold windows of 14 codes; a shorter umi_length reads the first umi_length + 2 of them"""
    return list(w) + [1] * (14 - len(w))


def ordinary(seed, n, five=False, ul=12, pos0=100_000, prefix="r", n_mol=None, flag=0):
    """n plain reads on one position: n_mol molecules (n // 3 unless given) of n_mol // 2 + 1 cells, about every third copy one base off"""
    rng = np.random.default_rng(seed)
    n_mol = max(1, n // 3) if n_mol is None else n_mol
    mols = umis(rng, n_mol, ul)
    cells = [barcode(rng) for _ in range(n_mol // 2 + 1)]
    rows = []
    for i in range(n):
        m = int(rng.integers(0, n_mol))
        w = near(mols[m], int(rng.integers(0, ul + 2))) if rng.random() < 0.35 else mols[m]
        rows.append(row(join(f"{prefix}{i}", fields(pad_window(w, ul), QS[int(rng.integers(0, len(QS)))], five, cells[m % len(cells)]), tail=f"{i:x}"),
                        pos0, flag))
    return rows


def pair(rid, w, five, bc, f0=None, f1=None, q=("15", "14"), **kw):
    """two reads of one cell one base apart; f0 / f1 turn the (rid, field list) of each into a name"""
    out = []
    for c, (ww, qq, fn) in enumerate(((w, q[0], f0), (near(w, 6), q[1], f1 if f1 is not None else f0))):
        f = fields(ww, qq, five, bc)
        out.append(row(fn(f"{rid}c{c}", f) if fn is not None else join(f"{rid}c{c}", f, tail=f"{c:x}"), **kw))
    return out


# ---- marker_cases --------------------------------------------------------------------------------------------------------------------------
def marker_cases(five=False):
    rng = np.random.default_rng(101 + five)
    ws = umis(rng, 16)
    junk = "AE=1_PS=3_bc=" + "T" * 16 + "_ed=0_bcEnd=5_X=" + "C" * 43 + "_Q=3"
    rows = ordinary(102 + five, 9, five)
    # _FWD_ in front of a later _REV_: the _REV_ one counts, and the tags are read from there
    rows += pair("fr", ws[0], five, barcode(rng), lambda r, f: r + "_FWD_" + junk + join("", f, "_REV_"))
    # two _REV_ markers: the first one, and behind it the first occurrence of every tag
    rows += pair("rr", ws[1], five, barcode(rng), lambda r, f: join(r, f, "_REV_") + "_REV_" + junk + "_2b")
    # the marker at character 0
    rows += pair("", ws[2], five, barcode(rng), lambda r, f: join("", f, tail=r))
    # marker text inside the read id
    rows += pair("id", ws[3], five, barcode(rng), lambda r, f: join(r + "_FWD_x9", f))
    rows += pair("ie", ws[4], five, barcode(rng), lambda r, f: join(r + "_FWD", f, "_REV_"))
    # no marker at all (also: cut off, lower case): no flags, no position
    f = fields(ws[5], "15", five)
    rows += [row("plain" + join("", f, "_")), row(join("cut", f, "_FWD"[:4] + "x")), row(join("low", f, "_fwd_")), row("tiny"), row("_FWD"), row("_REV")]
    # a tag in front of the marker and again behind it with another value
    rows += pair("pre", ws[6], five, barcode(rng), lambda r, f: join(r + "_AE=1_bcEnd=700_Q=1_X=" + "G" * 43 + "_bc=" + "G" * 16 + "_ed=9", f))
    # a tag twice behind the marker: the first counts
    rows += pair("dup", ws[7], five, barcode(rng), lambda r, f: join(r, f + [("AE", "5"), ("bc", "G" * 16), ("bcEnd", "1"), ("X", "T" * 43), ("Q", "1"), ("ed", "7"),
                                                                            ("PS", "1")]))
    return finish(rows, five_prime=five)


# ---- tag_order_cases -----------------------------------------------------------------------------------------------------------------------
SEVEN = ["AE", "PS", "ed", "bc", "bcEnd", "X", "Q"]


def tag_orders():
    """the seven tags in seven orders: every tag is the last field once (rotations of a shuffled order), plus bcEnd in front of bc"""
    base = ["X", "bcEnd", "Q", "AE", "bc", "PS", "ed"]
    return [base[k:] + base[:k] for k in range(7)] + [list(reversed(SEVEN))]


def tag_order_cases(five=False):
    rng = np.random.default_rng(111 + five)
    ws = umis(rng, 16)
    rows = ordinary(112 + five, 9, five)
    for n, order in enumerate(tag_orders()):
        def f_order(r, f, order=order):
            d = dict(f)
            d.setdefault("PS", "700")
            return join(r, [(t, d[t]) for t in order], tail=None)      # the last tag's value ends with the name
        rows += pair(f"o{n}", ws[n], five, barcode(rng), f_order)
    # ed_sec= in front of ed=; bcStart= absent; unknown fields between the known ones
    def swap(r, f):
        d = dict(f)
        return join(r, [("T", "12"), ("AE", d["AE"]), ("PS", "700"), ("rk", "4"), ("ed_sec", "3"), ("ed", "0"), ("bc", d["bc"]), ("PE", "730"), ("bcEnd", d["bcEnd"]),
                        ("X", d["X"]), ("Q", d["Q"])])
    rows += pair("sw", ws[9], five, barcode(rng), swap)
    rows += pair("nb", ws[10], five, barcode(rng), lambda r, f: join(r, [(t, v) for t, v in f if t != "bcStart"]))
    rows += pair("wb", ws[11], five, barcode(rng), lambda r, f: join(r, [(t, v) for t, v in f if t != "bcStart"] + [("bcStart", "9")]))
    return finish(rows, five_prime=five)


# ---- number_cases --------------------------------------------------------------------------------------------------------------------------
EDGE_INTS = ["0", "-0", "-5", str(INT_MAX), str(INT_MIN)]


def number_cases(five=False, limit=-1):
    rng = np.random.default_rng(121 + five)
    ws = umis(rng, 24)
    rows = ordinary(122 + five, 9, five)
    for n, v in enumerate(EDGE_INTS):
        f = dict(fields(ws[n], "15", five, barcode(rng)))
        f.setdefault("PS", "700")
        rows.append(row(join(f"ps{n}", list({**f, "PS": v}.items()))))
        rows.append(row(join(f"be{n}", list({**f, "bcEnd": v}.items()))))
    # AE at 1, 5 and 10 digits with the window kept in place (bcEnd follows AE): pairs that cluster
    for n, ae in enumerate([7, 12345, 1234567890] + ([] if five else [INT_MAX])):
        end = ae + 16 if five else ae + 3 - POS
        rows += pair(f"ae{n}", ws[8 + n], five, barcode(rng), lambda r, f, ae=ae, end=end: join(r, [(t, str(ae) if t == "AE" else str(end) if t == "bcEnd" else v) for t, v in f]))
    rows.append(row(join("aemax", fields(ws[12], "15", five, barcode(rng), AE=str(INT_MAX)))))     # 5': the read position wraps as a Java int does
    # texts that are no numbers: the field is absent
    f = dict(fields(ws[13], "15", five, barcode(rng)))
    f.setdefault("PS", "700")
    rows.append(row(join("psx", list({**f, "PS": "12x"}.items()))))       # no PS: no position in 3', still one in 5'
    rows.append(row(join("edx", list({**f, "ed": "x"}.items()))))         # no barcode
    rows.append(row(join("bex", list({**f, "bcEnd": "x"}.items()))))      # HAS_BC without a window
    # ed at the limit and one above it
    for n, ed in enumerate(sorted({0, 1, 2, max(limit, 0), max(limit, 0) + 1})):
        rows += pair(f"ed{n}", ws[14 + n], five, barcode(rng), lambda r, f, ed=ed: join(r, [(t, str(ed) if t == "ed" else v) for t, v in f]))
    return finish(rows, five_prime=five, bc_edit_limit=limit)


# ---- q_cases -------------------------------------------------------------------------------------------------------------------------------
Q_FORMS = [("12", "11.9"), ("12.3", "12.2"), (".5", "0.4"), ("7.", "6.9"), ("007.25", "7.2"), ("1234.567", "1234.5"), ("0", "0.1")]


def q_groups(five=False, exchanged=False):
    """per form a set of two reads of one cell one base apart: the clusterer takes the read of the higher quality for the centre"""
    rng = np.random.default_rng(131 + five)
    ws = umis(rng, len(Q_FORMS))
    out = []
    for n, (form, other) in enumerate(Q_FORMS):
        q = (other, form) if exchanged else (form, other)
        out.append(pair(f"q{n}", ws[n], five, barcode(rng), q=q))
    return out


def q_cases(five=False, exchanged=False):
    rows = ordinary(132 + five, 9, five)
    for g in q_groups(five, exchanged):
        rows += g
    return finish(rows, five_prime=five)


def q_group_rows():
    """chunk indices of the members of every q group"""
    return [(9 + 2 * n, 10 + 2 * n) for n in range(len(Q_FORMS))]


# ---- window_cases --------------------------------------------------------------------------------------------------------------------------
def bc_end_for(pos, five, ae):
    return ae - 3 + pos if five else ae + 3 - pos


def window_cases(five=False, ul=12):
    rng = np.random.default_rng(141 + five + ul)
    ws = umis(rng, 12, ul)
    ae = 50 if five else 743
    rows = ordinary(142 + five, 9, five, ul)
    last = X_LEN - ul - 1                                # pos + umi_length + 1 == len(X)

    def pair_at(rid, w, pos, x=None):
        out = []
        for c, ww in enumerate((w, near(w, 3))):
            xx = window_x(ww, five, pos) if x is None else x
            out.append(row(join(f"{rid}c{c}", fields(pad_window(ww, ul), ("15", "14")[c], five, bc, bcEnd=str(bc_end_for(pos, five, ae)), X=xx))))
        return out
    for n, pos in enumerate((0, 1, last, last + 1)):    # none, the first legal one, the last legal one, none
        bc = barcode(rng)
        rows += pair_at(f"w{n}", ws[n], pos)
    bc = barcode(rng)
    rows += pair_at("xe", ws[4], POS, x="")            # X= empty
    # N and lower-case letters inside the window: code 15, N in U7
    bc = barcode(rng)
    for c, ww in enumerate((ws[5], near(ws[5], 3))):
        x = list(window_x(pad_window(ww, ul), five))
        for k in (2, 5):
            i = POS - 1 + k if five else X_LEN - (POS + k)
            x[i] = "N" if k == 2 else x[i].lower()
        rows.append(row(join(f"xn{c}", fields(pad_window(ww, ul), "15", five, bc, X="".join(x)))))
    rows += pair("nq", ws[6], five, barcode(rng), lambda r, f: join(r, [(t, v) for t, v in f if t != "Q"]))       # X= without Q=: no window, HAS_BC stays
    rows += pair("nc", ws[7], five, barcode(rng), lambda r, f: join(r, [(t, v) for t, v in f if t != "bc"]))      # ed= without bc=
    return finish(rows, five_prime=five, umi_length=ul)


def window_pos_limits(ul):
    return dict(first_legal=1, last_legal=X_LEN - ul - 1, first_illegal=X_LEN - ul)


# ---- cigar_cases ---------------------------------------------------------------------------------------------------------------------------
C1 = [("S", 30), ("M", 100), ("N", 500), ("M", 50), ("I", 3), ("M", 20), ("D", 2), ("M", 40), ("S", 10)]   # blocks: reads 31-130, 131-180, 184-203, 204-243
C_ODD = [("S", 30), ("M", 100), ("I", 3), ("N", 6), ("M", 50)]      # reference gap in front of the second block: 7
C_EVEN = [("S", 30), ("M", 100), ("I", 3), ("N", 7), ("M", 50)]     # ... 8
C_EQX = [("S", 10), ("=", 40), ("X", 5), ("=", 60)]
C_HP = [("H", 5), ("S", 30), ("M", 100), ("P", 4), ("M", 50), ("H", 5)]


def cigar_probes():
    """(label, cigar, read position, flag, alignment start parity): `wrong` is where a walk that misses the rule would put the read"""
    p = []
    add = lambda label, cig, rp, flag=0, odd=False: p.append(dict(label=label, cigar=cig, rp=rp, flag=flag, odd=odd))  # noqa: E731
    add("zero", C1, 0)
    add("negative", C1, -7)
    add("lead_s_even", C1, 10)
    add("lead_s_odd", C1, 10, odd=True)
    add("in_i_gap1", C1, 182)
    add("in_i_gap7", C_ODD, 132)
    add("in_i_gap8", C_EVEN, 132)
    add("block_first", C1, 31)
    add("block_last", C1, 130)
    add("behind_n", C1, 131)
    add("block2_last", C1, 180)
    add("behind_i", C1, 184)
    add("behind_d", C1, 204)
    add("last_base", C1, 243)
    add("eq_first", C_EQX, 11)
    add("x_inside", C_EQX, 52)
    add("eq_second", C_EQX, 60)
    add("h_ignored", C_HP, 31)
    add("p_ignored", C_HP, 131)
    add("behind_299", C1, 542)
    add("behind_300", C1, 543)
    add("no_cigar_near", [], 200)
    add("no_cigar_far", [], 600)
    add("unmapped", C1, 100, flag=4)
    add("reverse_alone", C1, 100, flag=16)
    add("reverse_with_anchors", C1, 100, flag=16)
    return p


def probe_name(rid, rp, w, five, bc, ul=12):
    """the one name of cigar_cases: only PS= (3') or AE= (5', with bcEnd behind it so that the window stays) moves the read position"""
    if five:
        ae = rp - 16 - ul - 100
        return join(rid, fields(w, "15", True, bc, AE=str(ae), bcEnd=str(ae + 16)))
    return join(rid, fields(w, "15", False, bc, PS=str(rp + 100)))


def cigar_layout(five=False):
    """-> rows and, per probe and copy, dict(label, probe row, anchor rows, expect 'with' / 'without' the anchors, the walk's arguments).  An
    anchor is a 1000M read grouped by its first base.  ReadGrouper never takes the first read behind a gap into a chain, and a chain link must be
    shorter than 500.  So a probe with a position P stands once as [one read at P - 10, the probe, three anchors at P + 499] and once as [four
    anchors at P - 499, the probe]: one base down in the first copy or up in the second breaks the link of 499, and some read's region changes.
    A probe without a position stands behind four anchors put 10 in front of `where`, the place a walk that misses the rule would give it."""
    import pymodel_group as pg

    rng = np.random.default_rng(151 + five)
    rows, groups = [], []
    anchor_w = umis(rng, 1)[0]
    for g, pr in enumerate(cigar_probes()):
        w, bc = umis(rng, 1)[0], barcode(rng)
        for s in range(2):
            base = 1_000_000 + 40_000 * g + 20_000 * s + (1 if pr["odd"] else 0)      # pos0 of the probe: its alignment starts at base + 1
            walked = pg.ref_position_at_read_position(pr["cigar"], base + 1, pr["rp"])
            P = None if pr["flag"] & 4 else walked
            expect = "with" if P is not None and pr["label"] != "reverse_alone" else "without"
            where = P if P is not None else walked if walked is not None else \
                {"zero": base + 1 - base // 2, "behind_300": base + 1 + 711, "no_cigar_far": 1}[pr["label"]]
            if s == 1 and (expect == "without" or where < 600):
                continue
            a_flag = 16 if pr["label"] == "reverse_with_anchors" else 0
            anchor = lambda k, at: row(probe_name(f"an{g}s{s}k{k}", 1, anchor_w, five, BC0), at - 1, a_flag)  # noqa: E731
            t = row(probe_name(f"pr{g}s{s}", pr["rp"], w, five, bc), base, pr["flag"], pr["cigar"])
            if expect == "with" and s == 0:
                block = ([anchor(3, where - 10)] if where >= 20 else []) + [t] + [anchor(k, where + 499) for k in range(3)]
            elif expect == "with":
                block = [anchor(k, where - 499) for k in range(4)] + [t]
            elif where >= 20:
                block = [anchor(k, where - 10) for k in range(4)] + [t]
            else:
                block = [t] + [anchor(k, where + 10) for k in range(4)]
            first = len(rows)
            rows += block
            groups.append(dict(label=pr["label"], probe=first + block.index(t), anchors=[first + k for k, x in enumerate(block) if x is not t],
                               expect=expect, exact=where >= 20, shift=(-1, 1)[s], where=where, cigar=pr["cigar"], start=base + 1, rp=pr["rp"],
                               flag=pr["flag"]))
    return rows, groups


def cigar_cases(five=False):
    return finish(cigar_layout(five)[0], five_prime=five)


# ---- long_name_cases -----------------------------------------------------------------------------------------------------------------------
def _to_length(rid, f, n, marker="_FWD_"):
    """the name of exactly n characters: the read id is stretched"""
    short = join(rid, f, marker)
    assert len(short) <= n, (len(short), n)
    return join(rid + "k" * (n - len(short)), f, marker)


def _marker_at(rid, f, at, marker="_FWD_"):
    """the name whose marker starts at character `at`"""
    assert len(rid) <= at
    return join(rid + "k" * (at - len(rid)), f, marker)


def long_block(seed, five=False):
    """64 names of more than FLAT_LIMIT bytes in all"""
    rng = np.random.default_rng(seed)
    rows = []
    ws = umis(rng, 40)
    n_w = [0]

    def two(make):
        w, bc = ws[n_w[0]], barcode(rng)
        n_w[0] += 1
        for c, ww in enumerate((w, near(w, 6))):
            rows.append(row(make(f"l{n_w[0]}c{c}", fields(ww, ("15", "14")[c], five, bc))))
    # names of 30 characters: a position (3': PS) and nothing else
    for k in range(4):
        nm = (f"s{k}_FWD_PS=700_AE=743_" + "z" * 30)[:30]
        assert len(nm) == 30
        rows.append(row(nm))
    for n in (NAME_STAGE, NAME_STAGE + 1, NAME_STAGE + 4):                 # exactly 320, 321, 324 characters
        two(lambda r, f, n=n: _to_length(r, f, n))
    for _ in range(9):                                                     # about 700 characters, the marker behind character 320
        two(lambda r, f: _marker_at(r, f, 540 + int(rng.integers(0, 30))))
    fill = ("fill", "g" * 380)
    for _ in range(7):                                                     # the marker in front, every tag behind character 320
        two(lambda r, f: join(r, [fill] + f + [fill]))
    x_at = lambda f: len("_".join(f"{t}={v}" for t, v in f[:[t for t, _ in f].index("X")])) + 1 + 2   # noqa: E731  offset of X='s value behind the marker's end
    for start in (NAME_STAGE - 17, NAME_STAGE - 10, NAME_STAGE - 30, NAME_STAGE - 42):     # X= straddles character 320 (at -17: inside the 3' window)
        two(lambda r, f, start=start: _marker_at(r, f, start - x_at(f) - 5))
    for marker, at in (("_REV_", NAME_STAGE - 3), ("_FWD_", NAME_STAGE - 4), ("_REV_", NAME_STAGE - 1), ("_REV_", NAME_STAGE)):   # _RE | V_, _FWD | _, _ | REV_, | _REV_
        two(lambda r, f, marker=marker, at=at: _marker_at(r, f, at, marker))
    while len(rows) < 64:
        two(lambda r, f: _marker_at(r, f, 400 + int(rng.integers(0, 100))))
    assert len(rows) == 64
    return rows


def long_name_cases(which="a", five=False, seed=0):
    if which == "a":
        return finish(long_block(161 + five, five), five_prime=five)
    if which == "b":           # three waves: flat, not flat, a partial flat one
        rows = ordinary(162 + five, 64, five) + long_block(163 + five, five) + ordinary(164 + five, 7, five, prefix="t")
        kw = dict(random_umi_seed=seed) if seed else {}
        return finish(rows, five_prime=five, **kw)
    # c: a flat wave with one name of 900 characters among 63 short ones: the names behind it lie far from their lane's usual place in LDS
    rng = np.random.default_rng(166 + five)
    rows = ordinary(165 + five, 64, five)
    rows[5:7] = pair("big", umis(rng, 1)[0], five, barcode(rng), lambda r, f: _to_length(r, f, 900), lambda r, f: join(r, f))
    assert len(rows) == 64 and len(rows[5]["name"]) == 900
    return finish(rows, five_prime=five)


# ---- tail_cases ----------------------------------------------------------------------------------------------------------------------------
TAIL_CUTS = [1, 2, 63, 64, 65, 128, 129, 255, 256, 257]


def tail_records(five=False):
    """300 records, 20 per position, the positions 2,000 apart in coordinate order; some carry no marker or are unmapped, but never the last of a cut"""
    rows = []
    for locus in range(15):
        rows += ordinary(171 + locus + 100 * five, 20, five, pos0=100_000 + 2_000 * locus, prefix=f"t{locus}x", n_mol=5)
    keep = {c - 1 for c in TAIL_CUTS}
    for i, r in enumerate(rows):
        if i in keep:
            continue
        if i % 7 == 3:
            r["name"] = f"plain{i}"
        elif i % 11 == 5:
            r["flag"] |= 4
    return rows


def tail_cases(n=64, five=False, keep_data_end=False):
    kw = dict(keep_data_end=True) if keep_data_end else {}
    return finish(tail_records(five)[:n], five_prime=five, **kw)


# ---- group_key_cases -----------------------------------------------------------------------------------------------------------------------
def group_key_layout(five=False):
    """-> rows, dict(name of the set -> chunk indices)"""
    rng = np.random.default_rng(181 + five)
    ws = umis(rng, 40)
    rows, sets = [], {}
    n_w = [0]

    def members(label, bc, k, pos0=100_000, mutual=False):
        w = ws[n_w[0]]
        n_w[0] += 1
        out = []
        for c in range(k):
            ww = w if c == 0 else near(w, 6, c) if mutual else near(w, 3 + c)
            out.append((label, row(join(f"{label}c{c}", fields(ww, QS[c % len(QS)], five, bc), tail=f"{c:x}"), pos0)))
        return out

    def put(items):
        for label, r in items:
            sets.setdefault(label, []).append(len(rows))
            rows.append(r)
    put(members("base", BC0, 3))
    put(members("first", "C" + BC0[1:], 3))                # differs in the first base only
    put(members("last", BC0[:-1] + "A", 3))                # ... in the last base only
    put(members("mid", BC0[:7] + "A" + BC0[8:], 3))        # ... in one middle base
    put(members("allA", "A" * 16, 3))                      # key 0
    put(members("allT", "T" * 16, 3))                      # key 0xFFFFFFFF: with the region in front it is not the ~0 of a record that takes no part
    put(members("one", barcode(rng), 1))                   # a set of one read is not clustered
    put(members("two", barcode(rng), 2))
    put(members("three", barcode(rng), 3))
    # two sets whose members alternate; three reads one base apart from each other: the centre is the first in input order
    a, b = members("ilA", barcode(rng), 3, mutual=True), members("ilB", barcode(rng), 3, mutual=True)
    put([x for ab in zip(a, b) for x in ab])
    put([("plain", row(f"noname{k}")) for k in range(3)])
    bc2 = barcode(rng)
    w2 = ws[n_w[0]]
    for r in ordinary(182 + five, 70, five):
        put([("fill", r)])
    # the same barcode and UMI in two regions 5,000 apart (the first read behind a gap never joins a chain: one read in front)
    put([("far_open", row(join("open", fields(ws[39], "15", five, barcode(rng))), 105_000))])
    for k in range(3):
        put([("sameA", row(join(f"sa{k}", fields(w2, QS[k], five, bc2), tail=f"{k:x}"), 100_000))])
    for k in range(3):
        put([("sameB", row(join(f"sb{k}", fields(w2, QS[k], five, bc2), tail=f"{k:x}"), 105_000))])
    for r in ordinary(183 + five, 12, five, pos0=105_000, prefix="u"):
        put([("fill2", r)])
    order = sorted(range(len(rows)), key=lambda i: rows[i]["pos0"])     # coordinate order, input order inside a position
    back = {old: new for new, old in enumerate(order)}
    return [rows[i] for i in order], {k: [back[i] for i in v] for k, v in sets.items()}


def group_key_cases(five=False):
    return finish(group_key_layout(five)[0], five_prime=five)


# ---- fallback_cases ------------------------------------------------------------------------------------------------------------------------
def _sub(tag, text):
    """replace the text of the first `tag` of a name"""
    return lambda nm: re.sub(r"_" + tag + r"=[^_]*", "_" + tag + "=" + text, nm, count=1)


# (id, edit of the one name, what the test holds the chunk to: 'model' = host path and model, 'error' = SmiError on both paths)
FALLBACKS = [
    ("bc15", _sub("bc", BC0[:15]), "model"),
    ("bc17", _sub("bc", BC0 + "A"), "model"),
    ("bcN", _sub("bc", BC0[:5] + "N" + BC0[6:]), "model"),
    ("ps_plus", _sub("PS", "+5"), "model"),
    ("ps_blank", _sub("PS", " 5"), "model"),
    ("q_exp", _sub("Q", "1e1"), "model"),
    ("q_neg", _sub("Q", "-1"), "model"),
    ("q_4dec", _sub("Q", "1.2345"), "model"),
    ("q_8dig", _sub("Q", "12345678"), "model"),
    ("q_29", _sub("Q", "12." + "0" * 26), "model"),                         # 29 characters
    ("ae_zeros", _sub("AE", "000000000743"), "model"),                      # 12 digits, the value 743
    ("bcend_11", _sub("bcEnd", "99999999999"), "model"),                    # outside int: no bcEnd
    ("ae_11", _sub("AE", "30000000743"), "error"),                          # outside int: no adapter end
    ("ae_absent", lambda nm: nm.replace("_AE=", "_AF=", 1), "error"),
    ("ae_12x", _sub("AE", "12x"), "error"),
    ("ends_in_rev", lambda nm: nm.split("_FWD_")[0] + "_REV_", "error"),
]
FALLBACK_AT = 10


def fallback_cases(which, name=None):
    """the ordinary chunk of 70 with one name edited (or, with `name`, replaced by that one)"""
    rows = ordinary(191, 70)
    before = rows[FALLBACK_AT]["name"]
    rows[FALLBACK_AT]["name"] = {k: f for k, f, _ in FALLBACKS}[which](before) if name is None else name
    assert rows[FALLBACK_AT]["name"] != before
    return finish(rows)


# ---- the registry --------------------------------------------------------------------------------------------------------------------------
def _cases():
    c = {}
    for five in (False, True):
        p = "5p" if five else "3p"
        c[f"marker-{p}"] = (marker_cases, dict(five=five))
        c[f"tag_order-{p}"] = (tag_order_cases, dict(five=five))
        for limit in (0, 1, -1):
            c[f"number-{p}-limit{limit}"] = (number_cases, dict(five=five, limit=limit))
        c[f"q-{p}"] = (q_cases, dict(five=five))
        for ul in (8, 10, 12):
            c[f"window-{p}-ul{ul}"] = (window_cases, dict(five=five, ul=ul))
        c[f"cigar-{p}"] = (cigar_cases, dict(five=five))
        for which in "abc":
            c[f"long-{which}-{p}"] = (long_name_cases, dict(which=which, five=five))
        c[f"group_key-{p}"] = (group_key_cases, dict(five=five))
    for n in TAIL_CUTS:
        c[f"tail-{n}"] = (tail_cases, dict(n=n, five=n % 2 == 0))
    return c


CASES = _cases()                                   # id -> (function, arguments): every chunk that must stay on the device


def case(cid):
    fn, kw = CASES[cid]
    return fn(**kw)
