"""Inputs of the record-reader tests (test infrastructure only): tiny BAMs, one per rule of LongreadRecord.fromSAMRecord and of the
four programs' filters, and what tests/isoformmodel.py, consensusmodel.py, collapsemodel.py and fusionmodel.py make of each.
tests/test_longread_cpu.py runs them through tools/asan/longread_host.cpp, tests/test_longread_edges_gpu.py through the four handles.

All four programs read the same tags here (BC U8 GE RN, as FusionDetector fixes them), so that every record means something to each."""
import re
import struct

import bammodel
import collapsemodel as colm
import consensusmodel as cm
import fusionmodel as fm
import isoformmodel as im
import tagbammodel as tm

PROGRAMS = ("isoform", "consensus", "collapse", "fusion")
TAGS = dict(cell_tag="BC", umi_tag="U8", gene_tag="GE", rn_tag="RN")
MAX_CLIP, RN_MIN = 150, 3
CC_CFG = dict(TAGS, tso_end_tag="TE", polya_start_tag="PS", cdna_tag="CS", us_tag="US", max_clip=MAX_CLIP, mapqv0=False)
ISO_CFG = dict(TAGS, max_clip=MAX_CLIP, mapqv0=False)
COL_CFG = dict(TAGS, iso_tag="IT", max_clip=MAX_CLIP, rn_min=RN_MIN)
CSV = "CELL1-1\nCELL2\nA-1-1\n--11\n"
HEAD = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr9\tLN:2000000\n"
REFS = [("chr9", 2000000)]
M100 = [("M", 100)]
# the record-level counters, under the names the handles and the models share
COUNTS = dict(isoform=("records", "valid", "unvalid", "mapqv0", "no_gene", "no_umi", "chimeria", "null"),
              consensus=("records", "valid", "unvalid", "mapqv0", "no_gene", "no_umi", "chimeria", "null"),
              collapse=("records", "kept", "null", "mapq0", "chimeric", "low_rn", "not_listed", "no_gene"),
              fusion=("records", "valid", "unvalid", "mapqv0", "no_gene", "no_umi", "chimeria", "null"))
MALFORMED = "malformed attributes"


def rec(name, ge="GA", bc="CELL1", umi="U", flag=0, mapq=60, rn=5, cs="ACGT", it="undef", cigar=None, ref_id=0, pos0=999, extra=b""):
    """a record every program keeps, unless an argument says otherwise (None: the attribute is left out)"""
    aux = b""
    for tag, v in (("BC", bc), ("U8", umi), ("GE", ge), ("CS", cs), ("IT", it)):
        if v is not None:
            aux += tm.aux_z(tag, v)
    if rn is not None:
        aux += tm.aux_int("RN", "C", rn)
    return bammodel.bam_record(name, flag, ref_id, pos0, mapq, M100 if cigar is None else cigar, "ACGT", aux=aux + extra)


def bam(records):
    return bammodel.bam_bytes(HEAD, REFS, records)


def _good(k):
    return [rec(f"g{k}_{i}") for i in range(2)]


def _one(r):
    """a good record in front of it and behind it: an error must name the middle one"""
    return bam(_good(0)[:1] + [r] + _good(1)[:1])


def _precedence():
    """every combination of the filters' reasons: what each program counts fixes the order of its tests"""
    out = []
    for mapq, flag in ((60, 0), (0, 0), (0, 0x100), (0, 0x800)):
        for clip in (None, 151, 10001):
            for ge in ("GA", "", "undef", None):
                for umi in ("U", None):
                    for bc in ("CELL1", "CELLX"):
                        for rn in (5, 2):
                            cig = M100 if clip is None else [("S", clip)] + M100
                            out.append(rec(f"p{len(out)}", ge=ge, bc=bc, umi=umi, flag=flag, mapq=mapq, rn=rn, cigar=cig))
    return bam(out)


def _threaded(errors=()):
    """8,200 records of mixed outcomes: three host threads at n_threads 4; `errors`: the records that carry an RN of type Z"""
    kinds = (dict(), dict(bc=None), dict(ge="undef"), dict(umi=None), dict(mapq=0, flag=0x100), dict(cigar=[("H", 10001)] + M100), dict(bc="CELLX"),
             dict(rn=1), dict(cigar=[("M", 40), ("N", 300), ("M", 60)]))
    out = []
    for i in range(8200):
        kw = dict(kinds[i % len(kinds)])
        if i in errors:
            kw = dict(rn=None, extra=tm.aux_z("RN", "7"))
        out.append(rec(f"t{i}", **kw))
    return bam(out)


def _us(us, te=None, ps=None, **kw):
    extra = tm.aux_z("US", us)
    if te is not None:
        extra += tm.aux_int("TE", "c", te)
    if ps is not None:
        extra += tm.aux_int("PS", "C", ps)
    return rec(kw.pop("name", "us"), cs=None, extra=extra, **kw)


# name -> (inflated BAM, keywords).  Keywords: malformed=<read>: the attributes of that read are damaged, which the Python models cannot
# say (they die on a Python exception, or read on): every program reports MALFORMED for it.  outside=<i>: record i's attributes are
# moved behind the segment in the index.
CASES = {
    # casts and nulls
    "rn_z_no_cell": (_one(rec("x", bc=None, rn=None, extra=tm.aux_z("RN", "7"))), {}),
    "rn_I_2_31": (_one(rec("x", rn=None, extra=tm.aux_int("RN", "I", 2 ** 31))), {}),
    "rn_I_max": (_one(rec("x", rn=None, extra=tm.aux_int("RN", "I", 2 ** 31 - 1))), {}),
    "rn_types": (bam([rec(f"x{c}", rn=None, extra=tm.aux_int("RN", c, 7)) for c in "cCsSiI"]), {}),
    "bc_i_unmapped": (_one(rec("x", bc=None, flag=4, extra=tm.aux_int("BC", "i", 3))), {}),
    "de_i_df_f": (_one(rec("x", extra=tm.aux_int("de", "i", 1) + tm.aux_f("df", 0.1))), {}),
    "df_z": (_one(rec("x", extra=tm.aux_z("df", "0.1"))), {}),
    "de_f_df_z": (_one(rec("x", extra=tm.aux_f("de", 0.1) + tm.aux_z("df", "0.1"))), {}),
    "bc_i_then_z": (_one(rec("x", bc=None, extra=tm.aux_int("BC", "i", 3) + tm.aux_z("BC", "CELL1"))), {}),
    "bc_z_then_i": (_one(rec("x", extra=tm.aux_int("BC", "i", 3))), {}),
    "no_cigar": (_one(rec("x", cigar=[])), {}),
    "no_cigar_unmapped": (_one(rec("x", cigar=[], flag=4)), {}),
    "no_sequence": (_one(rec("x", ref_id=-1)), {}),
    # damaged attributes
    "z_without_nul": (bam(_good(0) + [rec("x", extra=b"XZZabc")]), dict(malformed="x")),
    "b_of_type_x": (_one(rec("x", extra=b"XBBx" + struct.pack("<I", 1) + b"\0")), dict(malformed="x")),
    "b_past_the_end": (bam(_good(0) + [rec("x", extra=b"XBBi" + struct.pack("<I", 9) + b"\0" * 8)]), dict(malformed="x")),
    "two_bytes": (bam(_good(0) + [rec("x", extra=b"XY")]), dict(malformed="x")),
    "one_byte": (_one(rec("x", extra=b"X")), dict(malformed="x")),
    "i_cut_short": (bam(_good(0) + [rec("x", extra=b"XIi\1\0\0")]), dict(malformed="x")),
    "h_without_nul": (bam(_good(0) + [rec("x", extra=b"XHH1a")]), dict(malformed="x")),
    "b_seven_bytes": (_one(rec("x", extra=b"XBBc\0\0\0")), dict(malformed="x")),
    "b_count_max": (_one(rec("x", extra=b"XBBc" + struct.pack("<I", 0xffffffff) + b"\1\2\3")), dict(malformed="x")),
    "type_q": (_one(rec("x", extra=b"XYq\0\0\0\0")), dict(malformed="x")),
    # CIGAR and filter order
    "clip_no_block": (_one(rec("x", cigar=[("S", 10001)])), {}),
    "clip_no_block_151": (_one(rec("x", cigar=[("S", 151)])), {}),
    "clip_good": (bam([rec("a", cigar=[("S", 10001)] + M100), rec("b", cigar=M100 + [("H", 151)]), rec("c", cigar=[("S", 150)] + M100),
                       rec("d", cigar=[("H", 10000)] + M100)]), {}),
    "d_20_21": (bam([rec("d20", cigar=[("M", 50), ("D", 20), ("M", 50)]), rec("d21", cigar=[("M", 50), ("D", 21), ("M", 50)]),
                     rec("n", cigar=[("M", 50), ("N", 500), ("M", 30), ("I", 2), ("M", 20)])]), {}),
    "eq_x_blocks": (bam([rec("e", cigar=[("=", 50), ("X", 1), ("=", 49)]), rec("en", cigar=[("=", 50), ("N", 200), ("=", 50)])]), {}),
    "precedence": (_precedence(), {}),
    # ComputeConsensus' cDNA
    "no_cdna": (_one(rec("x", cs=None)), {}),
    "no_cdna_chimeric": (_one(rec("x", cs=None, cigar=[("S", 10001)] + M100)), {}),
    "te_negative": (_one(_us("ACGTACGTACGT", te=-1, name="x")), {}),
    "ps_cuts": (bam([_us("ACGTACGTACGT", te=2, ps=0, name="ps0"), _us("ACGTACGTACGT", te=2, ps=11, name="ps_last"),
                     _us("ACGTACGTACGT", te=2, ps=10, name="ps_in"), _us("ACGTACGTACGT", te=2, ps=200, name="ps_far"),
                     _us("ACGTACGTACGT", te=11, ps=5, name="te_behind"), _us("ACGTACGTACGT", name="bare")]), {}),
    "te_z": (_one(rec("x", cs=None, extra=tm.aux_z("US", "ACGTACGT") + tm.aux_z("TE", "1"))), {}),
    # the "-1" removal
    "minus1": (bam([rec(f"m{i}", bc=b) for i, b in enumerate(("A-1-1", "-1-1", "1-1", "--11", "CELL1-1", "CELL2"))]), {}),
    # one segment on three threads
    "threaded": (_threaded(), {}),
    "threaded_errors": (_threaded(errors=(4100, 8150)), {}),
    "outside": (bam([rec(f"o{i}") for i in range(8)]), dict(outside=5)),
}


def _parse(msg):
    m = re.match(r"read (.*?): (.*)$", msg, re.S)
    return ("error", m.group(1), m.group(2))


def _counts(program, cnt):
    return {k: cnt.get(k, 0) for k in COUNTS[program]}


def _junc(j):
    return "".join(f"{a}-{b}," for a, b in j)


def expected(name):
    """-> {program: ("refused", record) | ("error", read, text) | ("counts", counters, kept)}; kept: (read, barcode, cdna, junctions) per
    kept record in file order, with None where the program's model does not hold the field"""
    data, kw = CASES[name]
    if "outside" in kw:
        return {p: ("refused", kw["outside"]) for p in PROGRAMS}
    if "malformed" in kw:
        return {p: ("error", kw["malformed"], MALFORMED) for p in PROGRAMS}
    out = {}
    try:
        kept, cnt = im.parse_records(data, ISO_CFG)
        out["isoform"] = ("counts", _counts("isoform", cnt), [(k["name"], k["bc"], None, _junc(k["junc"])) for k in kept])
    except im.IsoformError as e:
        out["isoform"] = _parse(str(e))
    try:
        kept, cnt = cm.parse_records(data, CC_CFG)
        out["consensus"] = ("counts", _counts("consensus", cnt), [(k["name"], k["bc"].decode(), k["cdna"].decode(), None) for k in kept])
    except cm.ConsensusError as e:
        out["consensus"] = _parse(str(e))
    try:
        cnt = dict.fromkeys(colm.COUNT_KEYS, 0)
        genes = colm.load(data, {}, set(im.cell_list(CSV)), COL_CFG, cnt)
        kept = [(r["name"], r["barcode"], None, _junc(r["junctions"])) for lst in genes.values() for t in lst for r in t.evidence]
        out["collapse"] = ("counts", _counts("collapse", cnt), kept)
    except colm.CollapseError as e:
        out["collapse"] = _parse(str(e))
    try:
        cnt = dict.fromkeys(fm.COUNT_KEYS, 0)
        kept = fm.parse_records(data, cnt)
        out["fusion"] = ("counts", _counts("fusion", cnt), [(k["name"], k["bc"], None, None) for k in kept])
    except fm.FusionError as e:
        out["fusion"] = _parse(str(e))
    return out
