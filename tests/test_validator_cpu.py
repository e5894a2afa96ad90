"""The validator of CollapseModel without a GPU: tests/validatormodel.py against results written out by hand for the hand-built case of
tests/validatorcases.py, the BED text forms, the record forms, the messages of the package, and that every edge tests/test_validator_gpu.py
claims is really in its input (asserted with the model)."""
import importlib
import inspect

import pytest

import bammodel
import collapsecases as cc
import collapsemodel as cm
import validatorcases as vc
import validatormodel as vm


@pytest.fixture(scope="module")
def hand():
    return vm.collapse_model(vc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, vc.HAND_CAGE, vc.HAND_POLYA, vc.hand_short())


def _columns(txt):
    """{(gene, transcript): columns 13-19 of .txt}"""
    out = {}
    for line in txt.decode().split("\n")[1:-1]:
        f = line.split("\t")
        assert len(f) == 19 and all(f[k] in ("true", "false") for k in (13, 15, 17, 18))
        out[(f[0], f[1])] = (int(f[12]), f[13] == "true", int(f[14]), f[15] == "true", int(f[16]), f[17] == "true", f[18] == "true")
    return out


def test_hand_built_case_columns_written_out_by_hand(hand):
    out, cnt, v, supports, _genes = hand
    assert _columns(out[".txt"]) == vc.HAND_EXPECTED
    assert supports == vc.HAND_SUPPORT
    txt = out[".txt"].decode()
    assert txt.startswith(cm.LEGEND)
    nss = "novel_not_in_catalog\tat_least_one_novel_splicesite"
    assert f"GA\tNovel.6\tchr12\t+\t1000\t3030\t3\t2\t2\t{nss}\t1050-1501,1600-3001\t5\ttrue\t0\ttrue\t7\ttrue\ttrue\n" in txt
    assert f"GO\tNovel.20\tchrB\t-\t50\t529\t2\t2\t1\t{nss}\t100-500\t0\tfalse\t2147483647\tfalse\t2147483647\tfalse\tfalse\n" in txt
    assert f"GP\tNovel.22\tchrB\t+\t150\t629\t2\t2\t1\t{nss}\t200-600\t0\tfalse\t-2147483647\tfalse\t-29\ttrue\tfalse\n" in txt
    assert "GB\tTB1\tchr12\t-\t999\t4100\t4\t2\t1\tfull_splice_match\tgencode\t-\t0\ttrue\t-51\tfalse\t-50\ttrue\tfalse\n" in txt


def test_hand_built_case_gff_and_final_files(hand):
    out, _cnt, _v, _s, _g = hand
    gff = out[".gff"].decode()
    assert ('chr12\tsicelore\ttranscript\t1000\t5030\t.\t+\t.\tgene_id "GA"; transcript_id "Novel.2"; category "novel_in_catalog"; '
            'subcategory "combination_of_known_splicesites"; UMIs "2"; Cells "2"; novelJunctions "1100-5001"; supportingReads "3"; CAGEdist "0"; '
            'POLYAdist "20"; color "#c594e1";\n') in gff
    assert 'transcript_id "TB1"; category "full_splice_match"; subcategory "gencode"; UMIs "2"; Cells "1"; novelJunctions "-"; ' \
           'supportingReads "0"; CAGEdist "-51"; POLYAdist "-50"; color "#014e8e";\n' in gff
    # the final files: the known transcripts and the five valid novels, in output order
    want = ["TA1", "Novel.1", "Novel.6", "Novel.2", "Novel.4", "TB1", "TB2", "Novel.9"]
    flat = out[".final.refflat.txt"].decode().split("\n")[:-1]
    assert [ln.split("\t")[1] for ln in flat] == want
    assert "GA\tNovel.2\tchr12\t+\t1000\t5030\t1000\t5030\t2\t999,5000,\t1100,5030," in flat
    assert "GB\tNovel.9\tchr12\t+\t1000\t2729\t1000\t2729\t2\t999,2699,\t1100,2729," in flat
    tx = [ln.split('transcript_id "')[1].split('"')[0] for ln in out[".final.gff"].decode().split("\n") if "\ttranscript\t" in ln]
    assert tx == want
    assert out[".refflat.txt"].count(b"\n") == 20 and out[".final.refflat.txt"].count(b"\n") == 8


def test_hand_built_case_counts_statistics_and_messages(pkg, hand):
    _out, cnt, v, _s, _g = hand
    assert (v["valid_isoforms"], v["valid_evidences"]) == (8, 16)
    assert (v["gencode_valid"], v["gencode_valid_ev"], v["ckj_valid"], v["ckj_valid_ev"]) == (3, 5, 1, 2)
    assert (v["cks_valid"], v["cks_valid_ev"], v["nss_valid"], v["nss_valid_ev"]) == (1, 2, 3, 7)
    # 32 records; 14 keys (the 16 distinct junctions less chrB's two); hits = the supports summed; table: the power of two >= 28
    assert (v["short_records"], v["junction_keys"], v["junction_hits"], v["table_slots"]) == (32, 14, 18, 32)
    # boundaries looked up: every record on chr12 without flag 0x4: 25 of one boundary, j5001_eqx 2, j3001_3 2, gn3 3, q_zero 1 of its 3
    assert v["short_boundaries"] == 23 + 2 + 2 + 3 + 1 + 1
    assert (v["cage_references"], v["cage_entries"], v["polya_references"], v["polya_entries"]) == (1, 8, 2, 8)
    want = ["\tCells detected\t\t[3]", "Loader Bam Start...", "Loader Bam End...10", "Collapser Start...[10 total genes]",
            "\tPerform validation using provided CAGE bed, POLYA bed and SHORT read bam files",
            "BEDParser\tcage.bed\t[references=1,entries=8]", "BEDParser\tdir/polya.bed\t[references=2,entries=8]",
            "Validator Start...[10 total genes]", "Printing statistics...",
            "-----------------------------------------------------------------------",
            "\t\t\t\t\tall_set (UMI)\tvalid_set (UMI)", "total_genes\t\t\t\t10", "total_isoforms\t\t\t\t20 (41)\t8 (16)", "full_splice_match",
            " o gencode\t\t\t\t3 (5)\t3 (5)", "novel_in_catalog", " o combination_of_known_junctions\t1 (2)\t1 (2)",
            " o combination_of_known_splicesites\t1 (2)\t1 (2)", "novel_not_in_catalog", " o at_least_one_novel_splicesite\t15 (32)\t3 (7)",
            "------------------------------------------------------------------------"]
    assert vm.message_lines(cnt, v, "cage.bed", "dir/polya.bed") == want
    col = importlib.import_module("sicelore_amd.collapsemodel")
    assert col.statistics_lines(cnt, v, "cage.bed", "dir/polya.bed") == want
    many = dict(cnt, genes=5001)
    lines = col.statistics_lines(many, v, "c", "p")
    assert lines == vm.message_lines(many, v, "c", "p") and lines[8:11] == ["2500 genes processed", "5000 genes processed", "Printing statistics..."]
    # without the validator's counts: today's lines
    assert "\tWon't perform validation (please provide CAGE bed, POLYA bed and SHORT read bam files" in col.statistics_lines(cnt)
    assert col.statistics_lines(cnt)[9] == "total_isoforms\t\t\t\t20 (41)\t3 (5)"


def test_public_interfaces_have_the_validator(pkg):
    col = importlib.import_module("sicelore_amd.collapsemodel")
    lib = importlib.import_module("sicelore_amd.lib")
    p = inspect.signature(col.collapse_model).parameters
    assert [p[k].default for k in ("cage", "polya", "short", "cage_co", "polya_co", "junc_co")] == [None, None, None, 50, 50, 1]
    assert all(hasattr(lib.Collapse, k) for k in ("validate_begin", "validate_segment", "validate_end", "validate_counts"))
    assert lib.COLLAPSE_VALIDATE_COUNTS == vm.VCOUNT_KEYS
    assert "validator" in col.__doc__ and "cli.py still refuses" in col.__doc__


@pytest.mark.parametrize("co", sorted(vc.HAND_VALID))
def test_hand_built_case_cut_offs(co):
    out, _cnt, v, _s, genes = vm.collapse_model(vc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, vc.HAND_CAGE, vc.HAND_POLYA, vc.hand_short(),
                                                cage_co=co[0], polya_co=co[1], junc_co=co[2])
    valid = [t.tx for g in sorted(genes) for t in genes[g] if t.is_novel and t.is_valid]
    assert valid == vc.HAND_VALID[co] and v["valid_isoforms"] == 3 + len(valid)
    cols = _columns(out[".txt"])
    # a junction with 0, juncCo - 1 and juncCo reads: 3100-4500 (0), 1100-2700 (2), 1100-5001 (3), 1100-2500 (1)
    assert cols[("GB", "Novel.9")][1] == (co[2] <= 2) and cols[("GA", "Novel.2")][1] and cols[("GA", "Novel.4")][1] == (co[2] <= 1)
    assert not cols[("GA", "Novel.5")][1] and cols[("GA", "TA1")][1]


def test_short_dictionary_with_chrB():
    """SHORT names chrB: chrB:100-500 and chr12:100-500 are two keys that differ in the reference id alone"""
    _out, _cnt, v, supports, _g = vm.collapse_model(vc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, vc.HAND_CAGE, vc.HAND_POLYA, vc.hand_short(True))
    assert supports[("chrB", 100, 500)] == 1 and supports[("chr12", 100, 500)] == 2 and supports[("chrB", 200, 600)] == 0
    assert v["junction_keys"] == 16 and v["junction_hits"] == 19


def test_without_the_three_inputs_the_model_is_todays():
    got = vm.collapse_model(vc.hand_bam(), cc.HAND_REF, cc.HAND_CSV)
    want = cm.collapse_model(vc.hand_bam(), cc.HAND_REF, cc.HAND_CSV)
    assert got[0] == want[0] and got[1] == want[1] and got[2] is None


# ---- BED ---------------------------------------------------------------------------------------------------------------------------------
def test_bed_text_forms():
    cage, n = vm.parse_bed(vc.HAND_CAGE, "CAGE")
    assert n == 8 and list(cage) == ["chr12"]
    assert cage["chr12"] == [(1000, 1010, "+"), (1500, 1510, "+"), (100, 110, "+"), (50, 60, None), (50, 50, None), (50, 60, None),
                             (4000, 4151, "-"), (4100, 4200, "+")]
    polya, n = vm.parse_bed(vc.HAND_POLYA, "POLYA")                 # CRLF
    assert n == 8 and list(polya) == ["chr12", "chrB"] and polya["chrB"] == [(600, 700, "+")] and polya["chr12"][6] == (900, 1049, "-")
    assert vm.parse_bed("chr1\t5\t9\r", "X")[0] == {"chr1": [(5, 9, None)]}               # a lone CR ends a line; no final line end needed
    assert vm.parse_bed("chr1 5 9 n 1e3 -  \n", "X")[0] == {"chr1": [(5, 9, "-")]}        # token 6 "-", then an empty token 7
    assert vm.parse_bed("chr1\t5\t9\tn\t.\t+\n", "X")[0] == {"chr1": [(5, 9, None)]}      # "." is no float
    assert vm.parse_bed("chr1\t5\t9\tn\tNaN\t+x\n", "X")[0] == {"chr1": [(5, 9, "+")]}    # the first character of the strand token
    assert vm.parse_bed("chr1\t5\t9\tn\t1\t+\t5\t9\tred\n", "X")[0] == {"chr1": [(5, 9, "+")]}
    assert vm.parse_bed("chr1\t5\t9\tn\t1\t+\t5\t9\t1,x\n", "X")[0] == {"chr1": [(5, 9, "+")]}   # NumberFormatException: black
    assert vm.parse_bed("chr1\t5\t9\tn\t1\t-\t5\t9\t0\t2\t2,2,\t0,2,\n", "X")[0] == {"chr1": [(5, 9, "-")]}
    with pytest.raises(vm.ValidatorError, match="X line 2:"):                             # a leading space makes an empty first token
        vm.parse_bed("\n chr1\t5\n", "X")
    assert vm.parse_bed("trackchr\t5\nbrowserx\t5\n#x\t5\nchr1\n\n", "X") == ({}, 0)


@pytest.mark.parametrize("which", sorted(vc.BAD_BED_LINES))
def test_bad_bed_line_fails_by_its_number(which):
    with pytest.raises(vm.ValidatorError, match=f"CAGE line {vc.BAD_BED_LINES[which][0]}:"):
        vm.parse_bed(vc.bad_cage(which), "CAGE")
    with pytest.raises(vm.ValidatorError, match=f"POLYA line {vc.BAD_BED_LINES[which][0]}:"):
        vm.collapse_model(vc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, vc.HAND_CAGE, vc.bad_cage(which), vc.hand_short())
    for text in ("chr1\t1\t1073741825\n", "chr1\t1\t2\tn\t0\t+\t1\t2\t0,0,256\n", "chr1\t1\t2\tn\t0\t+\t1\t2\t0\t-1\t1\t0\n"):
        with pytest.raises(vm.ValidatorError, match="X line 1:"):
            vm.parse_bed(text, "X")


def test_distance_rule():
    bed = vm.parse_bed(vc.HAND_CAGE, "CAGE")[0]
    pa = vm.parse_bed(vc.HAND_POLYA, "POLYA")[0]
    assert vm.distance(bed, "chr12", "+", 1000) == 0
    assert vm.distance(bed, "chr12", "+", 1550) == -50 and vm.distance(bed, "chr12", "+", 50) == 50     # never the '.' or two-token line at 50
    assert vm.distance(bed, "chr12", "+", 1551) == -51 and vm.distance(bed, "chr12", "+", 49) == 51
    assert vm.distance(bed, "chr12", "-", 4100) == -51                                                 # the - feature's end, not the + start 4100
    assert vm.distance(pa, "chr12", "+", 3030) == 7 and vm.distance(pa, "chr12", "+", 2529) == -7      # ties: the earlier line
    assert vm.distance(pa, "chrB", "-", 50) == vm.MAX_VALUE and vm.distance(bed, "chrB", "-", 50) == vm.MAX_VALUE
    assert vm.distance(bed, "chrB", "+", 50) == -vm.MAX_VALUE
    # the tie in both file orders on one position
    for text, want in (("c\t93\t99\tn\t0\t+\nc\t107\t109\tn\t0\t+\n", -7), ("c\t107\t109\tn\t0\t+\nc\t93\t99\tn\t0\t+\n", 7)):
        assert vm.distance(vm.parse_bed(text, "X")[0], "c", "+", 100) == want


# ---- SHORT -------------------------------------------------------------------------------------------------------------------------------
def test_block_boundaries():
    bj = vm.block_junctions
    p = 1000                                                    # pos0 = 999
    assert bj(p, [("M", 10), ("N", 100), ("M", 10)]) == [(999 + 10, 999 + 111)]
    assert bj(p, [("M", 10), ("D", 2), ("M", 10)]) == [(999 + 10, 999 + 13)]
    assert bj(p, [("M", 10), ("I", 1), ("M", 10)]) == [(1009, 1010)]
    assert bj(p, [("=", 5), ("X", 1), ("=", 5)]) == [(1004, 1005), (1005, 1006)]
    assert bj(p, [("M", 10), ("P", 1), ("M", 10)]) == [(1009, 1010)]
    assert bj(p, [("H", 5), ("S", 10), ("M", 51), ("D", 3900), ("P", 2), ("M", 30), ("S", 3)]) == [(1050, 4951)]
    assert bj(p, [("M", 100), ("M", 0), ("M", 0), ("M", 30)]) == [(1099, 1100)] * 3
    assert bj(p, []) == [] and bj(p, [("M", 50)]) == [] and bj(p, [("S", 5), ("N", 10)]) == []


def test_record_forms_are_in_the_hand_built_short():
    _t, refs, recs = bammodel.parse_bam(vc.hand_short())
    assert [r[0] for r in refs] == ["chrQ", "chr12"] and cc.REFS[0][0] == "chr12"         # another order than the ISOBAM's, and no chrB
    by = {r["name"]: r for r in recs}
    ops = lambda n: "".join(op for op, _l in by[n]["cigar"])  # noqa: E731
    assert ops("j5001_n") == "MNM" and ops("j5001_d") == "HSMDPMS" and ops("j5001_eqx") == "=IXN=" and ops("q_ins") == "MIM"
    assert by["q_zero"]["cigar"][1:3] == [("M", 0), ("M", 0)] and by["nocigar"]["cigar"] == [] and len(by["oneop"]["cigar"]) == 1
    assert by["j5001_unmapped"]["flag"] == 4 and by["j2700_sec"]["flag"] == 0x100 and by["j2500_sup"]["flag"] == 0x800
    assert by["j2700_dup"]["flag"] == 0x400 and by["j2700_dup"]["mapq"] == 0 and by["j5001_noref"]["ref_id"] == -1 and by["j5001_chrQ"]["ref_id"] == 0
    j = lambda n: vm.block_junctions(by[n]["pos0"] + 1, by[n]["cigar"])  # noqa: E731
    assert j("j5001_unmapped") == j("j5001_chrQ") == j("j5001_n") == j("j5001_d") == [(1100, 5001)] and j("j5001_eqx")[-1] == (1100, 5001)
    assert [j(f"j2500_off{k}")[0] for k in range(4)] == [(1099, 2500), (1101, 2500), (1100, 2499), (1100, 2501)]
    assert [j(f"j500_off{k}")[0] for k in range(4)] == [(103, 500), (105, 500), (104, 499), (104, 501)]
    assert j("q_zero") == [(7100, 7101)] * 3 and j("q_ins") == [(7100, 7101)] and j("pad") == [(3009, 3010)]


# ---- the edges tests/test_validator_gpu.py claims ------------------------------------------------------------------------------------------
def test_gpu_cases_hold_their_edges():
    # segments of 700 bytes cut the hand-built SHORT into several
    assert len(vc.hand_short()) > 3 * 700
    # 64 and 65 distinct keys
    for n in (64, 65):
        bam, ref, csv = vc.keys_case(n)
        _o, _c, v, sup, _g = vm.collapse_model(bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, vc.short_for_keys(n, [k % 4 for k in range(n)]))
        assert v["junction_keys"] == n and [sup[("chr12",) + vc.key_junction(k)] for k in range(n)] == [k % 4 for k in range(n)]
    # the long CIGAR
    bam, ref, csv, short, bounds = vc.long_cigar_case()
    _t, _r, recs = bammodel.parse_bam(short)
    assert len(recs[0]["cigar"]) == vc.LONG_OPS == 300 and vm.block_junctions(recs[0]["pos0"] + 1, recs[0]["cigar"]) == bounds and len(bounds) == 120
    assert set(op for op, _n in recs[0]["cigar"]) == set("HSMPIN")
    _o, _c, v, sup, _g = vm.collapse_model(bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, short)
    assert sup == {("chr12",) + bounds[k]: 1 for k in vc.LONG_KEYS} and v["short_boundaries"] == 120 and v["junction_hits"] == 4
    # keys that differ in one member
    bam, ref, csv, short = vc.near_keys_case()
    _o, _c, v, sup, _g = vm.collapse_model(bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, short)
    assert sup == {("chr12", 20050, 20081): 2, ("chrB", 20050, 20081): 1, ("chr12", 20051, 20081): 1, ("chr12", 20050, 20082): 0}
    # record counts around a wavefront and a block
    bam, ref, csv = vc.keys_case(3)
    for n in (0, 1, 63, 64, 65, 257):
        _o, _c, v, sup, _g = vm.collapse_model(bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, vc.short_sizes(n))
        assert v["short_records"] == n and v["junction_hits"] == n - n // 4 == v["short_boundaries"]
    # contention: 10,000 records on one key
    _o, _c, v, sup, _g = vm.collapse_model(*vc.keys_case(1), vc.FLAT_CAGE, vc.FLAT_CAGE, vc.short_for_keys(1, [10000]))
    assert sup == {("chr12",) + vc.key_junction(0): 10000}


def test_seeded_case_holds_its_edges():
    bam, ref, csv = cc.seeded_case(5)
    short, modes = vc.seeded_short(bam, ref, csv, 11)
    _t, _r, recs = bammodel.parse_bam(short)
    assert len(recs) == 20000 and sum(1 for r in recs if len(r["cigar"]) == 3) == 4000 and min(modes) > 800
    assert len(bammodel.bgzf_compress(short)) > 100000          # several segments of 100,000 and of 30,000 bytes
    _o, _c, v, sup, genes = vm.collapse_model(bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, short)
    n = len(sup)
    assert n > 60 and sum(1 for s in sup.values() if s > 0) >= n // 3 and sum(1 for s in sup.values() if s == 0) >= n // 4
    assert 0 < v["junction_hits"] < 4000 and v["short_boundaries"] == 4000
    assert any(t.is_novel and t.is_valid_junction and t.novel_junctions for g in genes for t in genes[g])
    assert any(t.is_novel and not t.is_valid_junction for g in genes for t in genes[g])
