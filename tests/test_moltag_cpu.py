"""The model of AddBamMoleculeTags / AddGeneNameTag (tests/moltagmodel.py) against outputs written out by hand and against the gene tagger's
own model (tests/genemodel.py), and the two sub-commands' parsing and refusals.  No GPU."""
import importlib
import struct

import pytest

import bammodel
import genemodel as gm
import moltagcases as mc
import moltagmodel as mm
import tagbammodel as tm


def test_split_rule_by_hand():
    want = {"A-B-3": ["A", "B", "3"], "A-B-3-": ["A", "B", "3"], "-B-3": ["", "B", "3"], "A--3": ["A", "", "3"], "A-B-3-4": None, "A-B": None,
            "A-": None, "-": None, "*": None, "A|B|3": ["A", "B", "3"], "A|B|3|": ["A", "B", "3"], "A|B-3": None, "|": None, "": None,
            "--": None, "a-b-3--": ["a", "b", "3"], "|B|3": ["", "B", "3"], "-|-": None, "X-Y--5": None, "X|Y|-5": None}
    for name, pieces in want.items():
        e = mm.name_edits(name)
        assert e == ([] if pieces is None else [("BC", pieces[0]), ("U8", pieces[1]), ("RN", int(pieces[2]))]), name
    assert mm.java_split("A-", "-") == ["A"] and mm.java_split("A-", "|") == ["A-"] and mm.java_split("-", "-") == [] and mm.java_split("", "-") == [""]
    e = mm.name_edits(mc.LONG_NAME)
    assert e == [("BC", "C" * 120), ("U8", "G" * 125), ("RN", 1234567)]


def test_integer_rule_by_hand():
    for s, v in (("007", 7), ("+7", 7), ("0", 0), ("2147483647", 2147483647), ("-2147483648", -2147483648), ("-0", 0)):
        assert mm.java_int(s) == v
    for s in ("2147483648", " 3", "3x", "", "+", "-", "3 ", "-2147483649", "1e3", "0x1", "+-1"):
        assert mm.java_int(s) is None, s
    for nm in mc.STOP_NAMES:
        with pytest.raises(ValueError):
            mm.name_edits(nm)


def test_smallest_integer_type_by_hand():
    want = {127: b"c\x7f", 128: b"C\x80", 255: b"C\xff", 256: b"s\x00\x01", 32767: b"s\xff\x7f", 32768: b"S\x00\x80", 65535: b"S\xff\xff",
            65536: b"i\x00\x00\x01\x00", 2147483647: b"i\xff\xff\xff\x7f", 0: b"c\x00", -1: b"c\xff", -129: b"s\x7f\xff", 2 ** 32 - 1: b"I\xff\xff\xff\xff"}
    for v, raw in want.items():
        assert mm.int_field(v) == raw, v


def test_attribute_list_by_hand():
    aux = tm.aux_z("ZZ", "last") + tm.aux_int("RN", "I", 70000) + tm.aux_h("XH", "0aFF") + tm.aux_z("AA", "first") + tm.aux_int("NM", "i", 2) + tm.aux_z("RN", "dup")
    got = mm.edit_aux(aux, [("BC", "ACGT"), ("U8", ""), ("RN", 300)])
    assert got == (b"U8Z\0" + b"AAZfirst\0" + b"BCZACGT\0" + b"XHBc\x02\0\0\0\x0a\xff" + b"NMc\x02" + b"RNs\x2c\x01" + b"ZZZlast\0")
    # binary-tag order: the SECOND character is the high byte ("U8" = 0x3855 sorts in front of "AA" = 0x4141)
    assert mm.edit_aux(tm.aux_z("AA", "x"), [("U8", "u")]) == b"U8Zu\0AAZx\0"
    assert mm.edit_aux(aux, [("XX", "a"), ("XX", "b")]).count(b"XXZ") == 1 and b"XXZb\0" in mm.edit_aux(aux, [("XX", "a"), ("XX", "b")])
    assert mm.edit_aux(tm.aux_z("GE", "g") + tm.aux_z("GS", "+"), [("XF", "UTR"), ("GE", None), ("GS", None), ("QQ", None)]) == b"XFZUTR\0"
    assert mm.edit_aux(b"", []) == b""
    mm.edit_aux(mc.many_attrs(61), [("BC", "a"), ("U8", "b"), ("RN", 1)])
    with pytest.raises(mm.BadAux):
        mm.edit_aux(mc.many_attrs(62), [("BC", "a"), ("U8", "b"), ("RN", 1)])
    for bad in (tm.aux_h("XH", "abc"), tm.aux_h("XH", "zz"), b"XXZnonul", b"XX", b"XXq\0"):
        with pytest.raises(mm.BadAux):
            mm.edit_aux(bad, [])


def test_molecule_tags_whole_bam_by_hand():
    bam = mc.bam_of([("chr1", 1000)], [mc.rec("ACGT-TTTT-300", [("M", 4)], 5, aux=tm.aux_z("BC", "old")), mc.rec("plain", [("M", 4)], 9, aux=tm.aux_z("BC", "old")),
                                       mc.rec("A|B|7", [("M", 4)], 1, ref=-1, flag=4)])
    out, cnt = mm.add_molecule_tags(bam)
    _t, _r, recs = bammodel.parse_bam(out)
    assert [r["aux"] for r in recs] == [b"U8ZTTTT\0BCZACGT\0RNs\x2c\x01", b"BCZold\0", b"U8ZB\0BCZA\0RNc\x07"]
    assert out[:mm.bammodel_records_start(bam)] == bam[:mm.bammodel_records_start(bam)] and cnt == dict(records=3, tagged=2)
    out, _ = mm.add_molecule_tags(bam, "XX", "XX", "RN")
    assert bammodel.parse_bam(out)[2][0]["aux"] == b"BCZold\0RNs\x2c\x01XXZTTTT\0"
    bad = mc.bam_of([("chr1", 1000)], [mc.rec("A-B-3", [("M", 4)]), mc.rec("A-B-3x", [("M", 4)]), mc.rec("A-B- 3", [("M", 4)])])
    with pytest.raises(mm.Stop) as e:
        mm.add_molecule_tags(bad)
    assert (e.value.read, e.value.record) == ("A-B-3x", 1)


@pytest.mark.parametrize("case", sorted(mc.GENE_CASES))
def test_gene_model_equals_the_taggers_model_under_default_options(case):
    """GE / GS / XF of every record = genemodel.tag (the model behind assignumis' tagger, pinned by ref_exec_gene.json)"""
    refflat, refs, records = mc.GENE_CASES[case]()
    bam = mc.bam_of(refs, records)
    out, cnt, decisions = mm.add_gene_name_tag(bam, refflat)
    tree, n = gm.load_refflat(refflat, [r[0] for r in refs])
    assert cnt["genes"] == n
    _t, _r, parsed = bammodel.parse_bam(bam)
    _t, _r, written = bammodel.parse_bam(out)
    assert len(parsed) == len(written) == len(records)
    for r, w, d in zip(parsed, written, decisions):
        if r["flag"] & 4 or r["ref_id"] < 0:
            assert d is None and w["aux"] == mm.edit_aux(r["aux"], [])
            continue
        ge, gs, xf = gm.tag(tree, refs[r["ref_id"]][0], r["flag"], r["pos0"], r["cigar"])
        got = mm.read_aux(w["aux"])
        assert (got.get(b"GE"), got.get(b"GS"), got.get(b"XF")) == tuple(None if v is None else b"Z" + v.encode() + b"\0" for v in (ge, gs, xf)), r["name"]


def test_gene_decisions_by_hand():
    refflat, refs, records = mc.locus_case()
    model = mm.GeneModel(refflat, [r[0] for r in refs])
    want = {"touchL": ("UTR", "F1"), "missL": ("INTRONIC", None), "touchR": ("CODING", "F1"), "missR": ("INTRONIC", None), "cdsL_hit": ("CODING", "F1"),
            "cdsL_miss": ("UTR", "F1"), "cdsR_hit": ("CODING", "F1"), "cdsR_miss": ("UTR", "F1"), "cds_in": ("CODING", "F1"), "nc_exon": ("UTR", "NC"),
            "nc_intron": ("INTRONIC", None), "intron": ("INTRONIC", None), "between": ("INTERGENIC", None), "two_a": ("CODING", "TWO"),
            "out_l": ("INTERGENIC", None), "out_in": ("CODING", "OUT"), "out_r": ("INTERGENIC", None), "out_split": ("INTRONIC", None),
            "both": ("CODING", "SMALL"), "both_utr": ("UTR", "SMALL"), "before": ("INTERGENIC", None), "cover": ("CODING", "F1"), "split": ("CODING", "F1")}
    _t, _r, parsed = bammodel.parse_bam(mc.bam_of(refs, records))
    seen = set()
    for r in parsed:
        if r["name"] in want:
            d = mm.gene_decision(model, refs[r["ref_id"]][0], r["flag"], r["pos0"], r["cigar"])
            assert (gm.NAMES[d["xf"]], ",".join(g.name for g in d["genes"]) or None) == want[r["name"]], r["name"]
            seen.add(r["name"])
    assert seen == set(want)


def test_strand_sets_options_and_metrics_by_hand():
    refflat, refs, records = mc.strand_case()
    bam = mc.bam_of(refs, records)
    out, cnt, dec = mm.add_gene_name_tag(bam, refflat)
    ge = {w["name"]: mm.read_aux(w["aux"]).get(b"GE") for w in bammodel.parse_bam(out)[2]}
    assert ge["same"] == b"ZP1\0" and ge["opposite"] is None and ge["both"] == b"ZP2\0" and ge["both_r"] == b"ZM2\0" and ge["none"] is None
    assert sorted(ge["three"][1:-1].split(b",")) == [b"D1", b"D2", b"D3"] and sorted(ge["two"][1:-1].split(b",")) == [b"D1", b"D2"]
    assert ge["three_r"] == b"ZD4\0" and sorted(ge["three_and_opp"][1:-1].split(b",")) == [b"D1", b"D2", b"D3"]
    assert cnt == dict(records=11, tagged=11, total_reads=11, wrong_strand=2, right_strand=9, ambiguous_fixed=4, ambiguous_rejected=0, multi_gene_records=4,
                       with_gene=8, genes=8)
    w = {x["name"]: x["aux"] for x in bammodel.parse_bam(out)[2]}
    assert w["opposite"] == b"XFZCODING\0ZZZkeep\0" and w["none"] == b"XFZINTERGENIC\0ZZZkeep\0"       # an input GE / GS disappears
    out, cnt, _ = mm.add_gene_name_tag(bam, refflat, use_strand=False)
    ge = {x["name"]: mm.read_aux(x["aux"]).get(b"GE") for x in bammodel.parse_bam(out)[2]}
    assert ge["opposite"] == b"ZM1\0" and sorted(ge["both"][1:-1].split(b",")) == [b"M2", b"P2"] and cnt["total_reads"] == cnt["right_strand"] == 0
    out, cnt, _ = mm.add_gene_name_tag(bam, refflat, allow_multi=False)
    assert all(b"GE" not in mm.read_aux(x["aux"]) and b"XF" in mm.read_aux(x["aux"]) for x in bammodel.parse_bam(out)[2])
    assert cnt["right_strand"] == cnt["total_reads"] == 11 and cnt["wrong_strand"] == cnt["with_gene"] == 0


def test_collision_pair_is_a_collision():
    refflat, refs, records, (a, b) = mc.collision_case()
    ha, hb = (gm.Gene("chrH", s, e, False, "x").hash() for s, e in (a, b))
    assert ha != hb and ((ha ^ (ha >> 16)) & 15) == ((hb ^ (hb >> 16)) & 15)
    out, cnt, _ = mm.add_gene_name_tag(mc.bam_of(refs, records), refflat)
    ge = {x["name"]: mm.read_aux(x["aux"])[b"GE"] for x in bammodel.parse_bam(out)[2]}
    assert ge["pair"] == b"ZHA,HB\0" or ge["pair"] == b"ZHB,HA\0"
    assert cnt["multi_gene_records"] == 2


def test_no_block_record():
    refflat, refs, records = mc.error_case(True)
    with pytest.raises(mm.Stop) as e:
        mm.add_gene_name_tag(mc.bam_of(refs, records), refflat)
    assert (e.value.read, e.value.record) == ("clipped", 1)
    refflat, refs, records = mc.error_case(False)
    out, _cnt, _ = mm.add_gene_name_tag(mc.bam_of(refs, records), refflat)
    assert bammodel.parse_bam(out)[2][1]["aux"] == b"XFZINTERGENIC\0"


def test_unsorted_header():
    hdr = mc.bam_of([("c", 5)], [])
    out = mm.unsorted_header(hdr)
    assert b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c\tLN:5\n" in out and out.endswith(hdr[8 + struct.unpack_from("<I", hdr, 4)[0]:])
    assert mm.unsorted_header(mc.bam_of([("c", 5)], [], head="")).startswith(b"BAM\1" + struct.pack("<I", 37) + b"@HD\tVN:1.6\tSO:unsorted\n@SQ")


# ---- the sub-commands ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module("sicelore_amd.cli")


def test_cli_parses_both_syntaxes(cli):
    a = cli._picard_parse(["-I", "a.bam", "-O", "b.bam", "-CELLTAG", "CB", "-UMITAG", "UB", "-RNTAG", "RX"], "AddBamMoleculeTags", cli.MT_OPTIONS, cli.MT_LONG)
    b = cli._picard_parse(["I=a.bam", "OUTPUT=b.bam", "CELLTAG=CB", "UMITAG=UB", "RNTAG=RX"], "AddBamMoleculeTags", cli.MT_OPTIONS, cli.MT_LONG)
    assert a == b == {"I": "a.bam", "O": "b.bam", "CELLTAG": "CB", "UMITAG": "UB", "RNTAG": "RX"}
    g = cli._picard_parse("-I a.bam -O b.bam -REFFLAT r -GENETAG GE -ALLOW_MULTI_GENE_READS true -USE_STRAND_INFO false -VALIDATION_STRINGENCY SILENT -DEBUG true"
                          .split(), "AddGeneNameTag", cli.GN_OPTIONS, cli.MT_LONG)
    assert g["USE_STRAND_INFO"] is False and g["ALLOW_MULTI_GENE_READS"] is True and g["GENETAG"] == "GE"
    assert {k: d for k, (_f, _k, d) in cli.GN_OPTIONS.items() if d is not None} == {
        "GENETAG": "GE", "STRANDTAG": "GS", "FUNCTIONTAG": "XF", "USE_STRAND_INFO": True, "ALLOW_MULTI_GENE_READS": True, "DEBUG": False,
        "VALIDATION_STRINGENCY": "STRICT"}
    assert {k: d for k, (_f, _k, d) in cli.MT_OPTIONS.items() if d is not None} == {"CELLTAG": "BC", "UMITAG": "U8", "RNTAG": "RN",
                                                                                   "VALIDATION_STRINGENCY": "STRICT"}


def test_cli_refusals(cli, tmp_path, capsys):
    bam = tmp_path / "in.bam"
    bam.write_bytes(b"")
    ref = tmp_path / "r.refFlat"
    ref.write_text("")
    cases = [
        (["AddBamMoleculeTags", "-I", str(bam)], "sub-command AddBamMoleculeTags: missing required option(s) O"),
        (["AddBamMoleculeTags", "-O", "x.bam"], "missing required option(s) I"),
        (["AddBamMoleculeTags", "-I", str(tmp_path / "nope.bam"), "-O", str(tmp_path / "o.bam")], f"AddBamMoleculeTags: I={tmp_path / 'nope.bam'}: no such file"),
        (["AddBamMoleculeTags", "-I", str(bam), "-O", str(tmp_path / "o.sam")], f"AddBamMoleculeTags: O={tmp_path / 'o.sam'}: this build writes BAM only"),
        (["AddBamMoleculeTags", "-I", str(bam), "-O", str(tmp_path / "no" / "o.bam")], "no such directory"),
        (["AddBamMoleculeTags", "-I", str(bam), "-O", str(tmp_path / "o.bam"), "-CELLTAG", "BCX"], "CELLTAG 'BCX' is not a two-character tag"),
        (["AddBamMoleculeTags", "-I", str(bam), "-O", str(tmp_path / "o.bam"), "-GENETAG", "GE"], "unknown option 'GENETAG'"),
        (["AddGeneNameTag", "-I", str(bam), "-O", str(tmp_path / "o.bam")], "sub-command AddGeneNameTag: missing required option(s) REFFLAT"),
        (["AddGeneNameTag", "-I", str(bam), "-O", str(tmp_path / "o.bam"), "-REFFLAT", str(tmp_path / "nope")], f"AddGeneNameTag: REFFLAT={tmp_path / 'nope'}: no such file"),
        (["AddGeneNameTag", "I=" + str(bam), "O=" + str(tmp_path / "o.txt"), "REFFLAT=" + str(ref)], "the output name must end in .bam"),
        (["AddGeneNameTag", "-I", str(bam), "-O", str(tmp_path / "o.bam"), "-REFFLAT", str(ref), "-USE_STRAND_INFO", "yes"], "USE_STRAND_INFO takes true or false"),
        (["NoSuchProgram"], "AddBamMoleculeTags, AddGeneNameTag"),
    ]
    for argv, msg in cases:
        assert cli.main(argv) == 1, argv
        assert msg in capsys.readouterr().err, argv
    assert not (tmp_path / "o.bam").exists()


def test_exports_and_header_agree(pkg):
    import os

    lib = importlib.import_module("sicelore_amd.lib")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sicelore_mi.h")).read()
    for name in ("smi_moltag_default_config", "smi_moltag_create", "smi_moltag_segment", "smi_moltag_counts", "smi_moltag_error_read",
                 "smi_moltag_stage_ms", "smi_moltag_free"):
        assert name in lib.EXPORTS and f"int {name}(" in header
    assert len(lib.MOLTAG_COUNTS) == int(header.split("#define SMI_MOLTAG_COUNTS ")[1].split()[0])
    assert len(lib.MOLTAG_STAGES) == int(header.split("#define SMI_MOLTAG_STAGES ")[1].split()[0])
    assert ctypes_size(lib.MolTagConfig) == 36


def ctypes_size(t):
    import ctypes

    return ctypes.sizeof(t)
