"""What smi_assignumis_chunk owes for a chunk, record by record, composed of pieces the suite already holds to the reference's bytecode or to
independent models -- test infrastructure only, and never through smi_assignumis_chunk itself:

  names      assignumis.scan_data_from_name (tests/test_ref_exec.py, tests/test_bam.py)
  windows    assignumis.umi_window (the same two files)
  positions  pymodel_group.ref_position_at_read_position (tests/test_group.py)
  regions    pymodel_group.group_sams (tests/test_group.py)
  U8 ...     the oracle's sor.umi_matrix and sor.umi_cluster_group on every (barcode, region) set of two or more reads with a window, members in
             input order (as tests/test_umi_gpu.py does)

Three things are added around scan_data_from_name, none of them a parser: Integer.parseInt decides what a number is (an optional number field
whose text it refuses counts as absent, an AE= it refuses as missing), the read id behind the last '_' is not looked at, and Java's int
arithmetic wraps."""
import importlib
import re

import numpy as np

import pymodel_group as pg

HAS_BC, HAS_U7, CLUSTERED, SKIPPED = 1, 2, 4, 8          # SMI_UMI_* of include/sicelore_mi.h
CIGAR_OPS = "MIDNSHP=X"
_DEC = {1: "A", 2: "G", 4: "C", 8: "T", 15: "N"}
_JAVA_INT = re.compile(r"[+-]?[0-9]+\Z")


def _au():
    return importlib.import_module("sicelore_amd.assignumis")


def java_int(text):
    """Integer.parseInt: the value, or None where it throws NumberFormatException"""
    if text is None or not _JAVA_INT.match(text):
        return None
    v = int(text)
    return v if -2 ** 31 <= v <= 2 ** 31 - 1 else None


def wrap32(v):
    """Java int arithmetic"""
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def scan(name, bc_edit_limit=None, strict=True):
    """scan_data_from_name of the name.  strict: Integer.parseInt decides what a number is (Python's int also reads blanks and any size): an AE=
    it refuses is the missing adapter end, PS= / ed= / bcEnd= values it refuses are struck out first, so that the field counts as absent -- the
    executed reference throws NumberFormatException in all four (tests/golden/ref_exec_umi_odd_names.json); for the three optional fields the
    product's reading is "no such field".  `_0` is put behind
    a name that has a marker: no value changes (a value ends at the next '_' or at the end of the name) and the read id, which nothing here uses,
    can be read."""
    au = _au()
    k = name.find("_REV_")
    if k < 0:
        k = name.find("_FWD_")
    if k < 0:
        return None                                # Optional.absent()
    if strict:
        head, sub = name[:k + 4], name[k + 4:]
        if java_int(au._extract(sub, "AE=")) is None:
            raise au._lib.SmiError("adapter position (AE=) not found in read name: " + name)
        for tag in ("PS=", "ed=", "bcEnd="):
            v = au._extract(sub, tag)
            if v is not None and java_int(v) is None:
                sub = sub.replace(tag, tag[:-1] + "~")
        name = head + sub
    return au.scan_data_from_name(name + "_0", None if bc_edit_limit is None or bc_edit_limit < 0 else bc_edit_limit)


def decode_cigar(raw):
    return [(CIGAR_OPS[int(c) & 15], int(c) >> 4) for c in np.asarray(raw, dtype=np.uint32)]


def read_position(d, five_prime, umi_length, grouping_distance):
    """the read position whose reference position the read is grouped by (NanoporeRead$ReadScanData L86-92), None without a polyA start in 3'"""
    if five_prime:
        return wrap32(wrap32(d["ae"]) + 16 + umi_length + grouping_distance)
    return None if d["ps"] is None else wrap32(wrap32(d["ps"]) - grouping_distance)


def splitmix(seed, k):
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(k) + 1)) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


def records(names, flags, pos0, cigars, five_prime=False, umi_length=12, bc_edit_limit=None, grouping_distance=100, random_umi_seed=0,
            strict=True, **_):
    """per record: dict(has_bc, bc, window (list of umi_length + 2 codes or None), q, position (or None), reverse)"""
    au = _au()
    out = []
    for i, nm in enumerate(names):
        d = scan(nm, bc_edit_limit, strict)
        r = dict(has_bc=False, bc=None, window=None, q=None, position=None, reverse=bool(int(flags[i]) & 16), read_pos=None)
        if d is not None:
            b = d["bc"]
            r["has_bc"] = b is not None and b["seq"] is not None
            r["bc"] = b["seq"] if r["has_bc"] else None
            r["q"] = d["q"]
            if r["has_bc"] and b["end"] is not None and d["x"] is not None and d["q"] is not None:
                r["window"] = au.umi_window(d["x"], d["ae"], b["end"], five_prime, umi_length)
                if r["window"] is not None and random_umi_seed:
                    z = splitmix(random_umi_seed, i)
                    r["window"] = [1 << ((z >> (2 * k)) & 3) for k in range(umi_length + 2)]
            rp = read_position(d, five_prime, umi_length, grouping_distance)
            r["read_pos"] = rp
            if rp is not None and not int(flags[i]) & 4:
                r["position"] = pg.ref_position_at_read_position(decode_cigar(cigars[i]), int(pos0[i]) + 1, rp)
        out.append(r)
    return out


def expect(sor, names, flags, pos0, cigars, max_dist=500, keep_data_end=False, umi_length=12, **kw):
    """-> (list of dict(region, center, u1, u2, flags, u8, u7) per record, n_done, the records() list)"""
    recs = records(names, flags, pos0, cigars, umi_length=umi_length, **kw)
    n = len(recs)
    region, n_done = pg.group_sams([r["position"] for r in recs], [r["reverse"] for r in recs], d=max_dist, keep_data_end=keep_data_end)
    tags = [dict(region=-1, center=-1, u1=-1, u2=-1, flags=0, u8="", u7="") for _ in range(n)]
    sets = {}
    for i in range(n_done):
        r, t = recs[i], tags[i]
        t["region"] = region[i]
        if r["has_bc"]:
            t["flags"] |= HAS_BC
        if r["window"] is not None:
            t["flags"] |= HAS_U7
            t["u7"] = "".join(_DEC[c] for c in r["window"][1:1 + umi_length])
            if region[i] >= 0:
                sets.setdefault((r["bc"], region[i]), []).append(i)
    for mem in sets.values():
        m = len(mem)
        if m < 2:                              # UmiClustering.lambda$cluster$6
            continue
        ws = np.array([recs[i]["window"] for i in mem], dtype=np.uint8)
        qv = np.array([recs[i]["q"] for i in mem], dtype=np.float32)
        asg, skipped = sor.umi_cluster_group(sor.umi_matrix(ws, umi_length).reshape(-1), m, qv)
        for j, i in enumerate(mem):
            t = tags[i]
            if asg["center"][j] < 0:
                if skipped[j]:
                    t["flags"] |= SKIPPED
                continue
            c, off = int(asg["center"][j]), int(asg["offset"][j])
            t["flags"] |= CLUSTERED
            t["center"], t["u1"], t["u2"] = mem[c], int(asg["ed"][j]), int(asg["ed_second"][j])
            t["u8"] = "".join(_DEC[int(ws[c][k + 1 + off])] for k in range(umi_length))
    return tags, n_done, recs


def long_names(names, stage):
    return sum(len(nm) > stage for nm in names)


def floors(tags, recs, names=(), stage=320):
    """what a chunk exercised: records with a window, with a position, inside a region, clustered, names longer than the LDS stage"""
    return dict(window=sum(r["window"] is not None for r in recs), position=sum(r["position"] is not None for r in recs),
                region=sum(t["region"] >= 0 for t in tags), clustered=sum(bool(t["flags"] & CLUSTERED) for t in tags), long=long_names(names, stage))


def least(cid):
    """the least a case of tests/uparsecases.py must exercise (tests/test_uparse_cases_cpu.py holds the model's counts to it, the GPU test the
    device's): a chunk that lost its windows, positions or sets would otherwise compare equal to a model that lost them too"""
    if cid in ("tail-1", "tail-2"):                      # one or two reads: no region (a chain needs three), nothing to cluster
        return dict(window=int(cid[5:]), position=int(cid[5:]), region=0, clustered=0, long=0)
    need = dict(window=10, position=10, region=10, clustered=10, long=0)
    if cid.startswith("long-"):
        need["long"] = 1 if cid.startswith("long-c") else 40
    return need


_CACHE = {}


def expected(sor, key, case, **extra):
    """expect() of a case of tests/uparsecases.py, computed once per session"""
    if key not in _CACHE:
        names, flags, pos0, cigars, kw = case
        _CACHE[key] = expect(sor, names, flags, pos0, cigars, **{**kw, **extra})
    return _CACHE[key]


def ref_position_branch(cigar, alignment_start, position):
    """which return of ref_position_at_read_position a call takes (the walk restated only to name the branch; the value is asserted against
    pg.ref_position_at_read_position where this is used): 'zero', 'in_front' (half-way rule), 'inside', 'behind_near', 'behind_far'"""
    if position == 0:
        return "zero"
    read_base, last_read_end = 1, 1
    for op, ln in cigar:
        if op in "SI":
            read_base += ln
        elif op in "M=X":
            if read_base + ln - 1 >= position:
                return "in_front" if position < read_base else "inside"
            last_read_end = read_base + ln - 1
            read_base += ln
    return "behind_near" if position - last_read_end < 300 else "behind_far"
