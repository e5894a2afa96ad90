"""CollapseModel without a GPU: tests/collapsemodel.py against output written out by hand for the hand-built case of
tests/collapsecases.py, the command line, and that every edge tests/test_collapse_gpu.py claims is really in its input (asserted with the
model, as tests/test_matrix_edges_cpu.py does for the matrices)."""
import importlib

import pytest

import bammodel
import collapsecases as cc
import collapsemodel as m

TAIL = "\t0\tfalse\t0\tfalse\t0\tfalse\tfalse\n"
NSS = "novel_not_in_catalog\tat_least_one_novel_splicesite"
# geneId transcriptId chrom strand txStart txEnd exons UMIs Cells categorie subcategorie novelJunctions, by hand from the records of
# collapsecases.hand_records (their comments say what each is there for)
HAND_TXT = m.LEGEND + "".join(row + TAIL for row in (
    "GA\tTA1\tchr12\t+\t999\t3100\t3\t2\t2\tfull_splice_match\tgencode\t-",
    "GA\tNovel.1\tchr12\t+\t1000\t5030\t3\t2\t1\tnovel_in_catalog\tcombination_of_known_junctions\t-",       # 1100-3001 is TA2's, 4100-5001 TA4's
    "GA\tNovel.5\tchr12\t+\t1550\t4529\t3\t2\t2\t" + NSS + "\t1600-3001,3100-4500",                            # known sites, then a novel site
    "GA\tNovel.6\tchr12\t+\t1000\t3030\t3\t2\t2\t" + NSS + "\t1050-1501,1600-3001",                            # a novel site, then known sites
    "GA\tNovel.2\tchr12\t+\t1000\t5030\t2\t2\t2\tnovel_in_catalog\tcombination_of_known_splicesites\t1100-5001",
    "GA\tNovel.4\tchr12\t+\t990\t2529\t2\t3\t3\t" + NSS + "\t1100-2500",                                       # Novel.3 had one record
    "GB\tTB1\tchr12\t-\t999\t4100\t4\t2\t1\tfull_splice_match\tgencode\t-",                                    # the last read's strand
    "GB\tTB2\tchr12\t+\t999\t3100\t2\t1\t1\tfull_splice_match\tgencode\t-",                                    # two exons: in front of Novel.9
    "GB\tNovel.9\tchr12\t+\t1000\t2729\t2\t2\t2\t" + NSS + "\t1100-2700",                                      # Novel.8 was inside TB1
    "GC1\tNovel.10\tchr12\t+\t50\t529\t2\t2\t1\t" + NSS + "\t100-500",                                         # a, b
    "GC1\tNovel.11\tchr12\t+\t50\t529\t2\t2\t1\t" + NSS + "\t104-500",                                         # c, d: 104 is 4 from 100
    "GC2\tNovel.12\tchr12\t+\t50\t529\t2\t3\t1\t" + NSS + "\t102-500",                                         # b founds: a and c both join
    "GD\tNovel.13\tchr12\t+\t50\t529\t2\t2\t1\t" + NSS + "\t100-500",                                          # d3 (102) joins the first
    "GD\tNovel.14\tchr12\t+\t50\t529\t2\t2\t1\t" + NSS + "\t104-500",
    "GN\tNovel.16\tchr12\t+\t1000\t4030\t4\t2\t1\t" + NSS + "\t1100-2001,2100-3001,3100-4001",
    "GN\tNovel.18\tchr12\t+\t1000\t2030\t2\t2\t1\t" + NSS + "\t1104-2001",                                     # inside the dropped Novel.17 only
    "GO\tNovel.20\tchrB\t-\t50\t529\t2\t2\t1\t" + NSS + "\t100-500",                                           # o1 is its last read
    "GO\tNovel.21\tchr12\t+\t50\t529\t2\t2\t1\t" + NSS + "\t104-500",
))
HAND_FINAL_REFFLAT = ("GA\tTA1\tchr12\t+\t999\t3100\t1050\t3050\t3\t999,2000,3000,\t1100,2100,3100,\n"
                      "GB\tTB1\tchr12\t-\t999\t4100\t999\t4100\t4\t999,2000,3000,4000,\t1100,2100,3100,4100,\n"
                      "GB\tTB2\tchr12\t+\t999\t3100\t999\t3100\t2\t999,3000,\t1100,3100,\n")
GFF_TB2 = ('chr12\tsicelore\ttranscript\t999\t3100\t.\t+\t.\tgene_id "GB"; transcript_id "TB2"; category "full_splice_match"; subcategory "gencode"; '
           'UMIs "1"; Cells "1"; novelJunctions "-"; supportingReads "0"; CAGEdist "0"; POLYAdist "0"; color "#014e8e";\n'
           'chr12\tsicelore\texon\t1000\t1100\t.\t+\t.\tgene_id "GB"; transcript_id "TB2";\n'
           'chr12\tsicelore\texon\t3001\t3100\t.\t+\t.\tgene_id "GB"; transcript_id "TB2";\n')
REFFLAT_NOVEL4 = "GA\tNovel.4\tchr12\t+\t990\t2529\t990\t2529\t2\t989,2499,\t1100,2529,\n"   # first start = min txStart, last end = max txEnd
GFF_NOVEL20 = ('chrB\tsicelore\ttranscript\t50\t529\t.\t-\t.\tgene_id "GO"; transcript_id "Novel.20"; category "novel_not_in_catalog"; '
               'subcategory "at_least_one_novel_splicesite"; UMIs "2"; Cells "1"; novelJunctions "100-500"; supportingReads "0"; CAGEdist "0"; '
               'POLYAdist "0"; color "#e65802";\n'
               'chrB\tsicelore\texon\t50\t100\t.\t-\t.\tgene_id "GO"; transcript_id "Novel.20";\n'
               'chrB\tsicelore\texon\t500\t529\t.\t-\t.\tgene_id "GO"; transcript_id "Novel.20";\n')


@pytest.fixture(scope="module")
def hand():
    return m.collapse_model(cc.hand_bam(), cc.HAND_REF, cc.HAND_CSV)


def test_hand_case_against_files_written_by_hand(hand):
    out, cnt, det = hand
    assert out[".txt"].decode() == HAND_TXT
    assert out[".final.refflat.txt"].decode() == HAND_FINAL_REFFLAT
    gff, flat = out[".gff"].decode(), out[".refflat.txt"].decode()
    assert GFF_TB2 in gff and GFF_TB2 in out[".final.gff"].decode() and GFF_NOVEL20 in gff and "Novel" not in out[".final.gff"].decode()
    assert REFFLAT_NOVEL4 in flat and flat.count("\n") == 18 and gff.count("\ttranscript\t") == 18
    assert out[".final.gff"].decode().count("\ttranscript\t") == 3
    # the loader: ten records of the filter's reasons, none of them evidence
    assert (cnt["records"], cnt["kept"], cnt["null"], cnt["mapq0"], cnt["chimeric"], cnt["low_rn"], cnt["not_listed"], cnt["no_gene"]) == \
        (59, 49, 2, 1, 1, 1, 2, 3)
    assert (cnt["genes"], cnt["founders"], cnt["novel_evidenced"], cnt["novel_filtered"], cnt["isoforms"], cnt["monoexon"]) == (8, 21, 19, 4, 18, 2)
    assert (cnt["gencode"], cnt["ckj"], cnt["cks"], cnt["nss"]) == (3, 1, 1, 13)
    assert det["GE"]["kept"] == [] and det["GE"]["founders"] == [("Novel.15", 1)]            # a gene left empty still counts
    assert det["GA"]["founders"][2] == ("Novel.3", 1) and det["GA"]["dropped"] == ["Novel.7"]  # MINEVIDENCE - 1; inside the unevidenced TA3
    assert det["GB"]["dropped"] == ["Novel.8"] and det["GN"]["dropped"] == ["Novel.17", "Novel.19"]
    assert det["GD"]["founders"] == [("Novel.13", 2), ("Novel.14", 2)]


def test_order_dependence_and_thresholds():
    out, _cnt, det = m.collapse_model(cc.hand_bam(order_gc2=("a", "b", "c")), cc.HAND_REF, cc.HAND_CSV)
    assert det["GC2"]["founders"] == [("Novel.12", 2), ("Novel.13", 1)]     # the same records as GC1's order: another result
    out3, cnt3, det3 = m.collapse_model(cc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, min_evidence=3)
    assert [k[0] for k in det3["GA"]["kept"]] == ["TA1", "Novel.4"] and [k[0] for k in det3["GC2"]["kept"]] == ["Novel.12"]  # at count
    _o, cnt4, det4 = m.collapse_model(cc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, min_evidence=4)
    assert [k[0] for k in det4["GA"]["kept"]] == ["TA1"] and cnt4["founders"] == 21                                        # at count + 1
    _o, cntr, _d = m.collapse_model(cc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, rn_min=2)
    assert cntr["low_rn"] == 54 and cntr["kept"] == 1                        # only a_known2 has RN 3; a missing RN counts as 1
    _o, cnt0, det0 = m.collapse_model(cc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, delta=0)
    assert det0["GC1"]["founders"] == [("Novel." + str(n), c) for n, c in ((11, 1), (12, 1), (13, 2))]


def test_loader_errors_name_the_read():
    recs = cc.hand_records()
    for bad, name in ((cc.rec("bad_it", cc.TA1, "GA", "TA9"), "bad_it"), (cc.rec("no_it", cc.TA1, "GA", None), "no_it"),
                      (cc.rec("zero_line", cc.TA1, "GZ", "TZ0"), "zero_line"),
                      (cc.rec("int_bc", cc.TA1, "GA", "TA1", bc=None, extra=cc.tm.aux_int("BC", "C", 3)), "int_bc"),
                      (cc.rec("z_rn", cc.TA1, "GA", "TA1", extra=cc.tm.aux_z("RN", "2")), "z_rn"),
                      (cc.rec("z_de", cc.TA1, "GA", "TA1", extra=cc.tm.aux_z("de", "0.1")), "z_de"),
                      (cc.rec("walk", [], "GA", "TA1", cigar=[("S", 40)]), "walk")):
        with pytest.raises(m.CollapseError) as e:
            m.collapse_model(bammodel.bam_bytes(cc.HEAD, cc.REFS, recs[:20] + [bad] + recs[20:]), cc.HAND_REF, cc.HAND_CSV)
        assert e.value.read == name
    # a bad ISOFORMTAG on a record the filter drops is never looked up; an unmapped record's de is never cast
    ok = [cc.rec("bad_it_mapq0", cc.TA1, "GA", "TA9", mapq=0), cc.rec("z_de_unmapped", cc.TA1, "GA", "TA1", flag=4, extra=cc.tm.aux_z("de", "x"))]
    m.collapse_model(bammodel.bam_bytes(cc.HEAD, cc.REFS, ok), cc.HAND_REF, cc.HAND_CSV)


def test_bad_refflat_line_fails_by_line():
    import isoformmodel as im

    for which, (no, bad) in cc.BAD_REF_LINES.items():
        with pytest.raises(im.IsoformError) as e:
            m.collapse_model(cc.hand_bam(), cc.bad_refflat(which), cc.HAND_CSV)
        assert f"REFFLAT line {no}:" in str(e.value), which
        assert cc.bad_refflat(which).split("\n")[no - 1] == bad and cc.bad_refflat(which).count("\n") == cc.HAND_REF.count("\n")
    assert m.parse_refflat(cc.HAND_REF)[1] == 6           # a well-formed line without exon bases (GZ) is left out, and is no error


# ---- the command line -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module("sicelore_amd.cli")


def test_cli_parses_both_syntaxes_and_defaults(cli):
    a = cli._picard_parse("-I a.bam -REFFLAT r -CSV c -OUTDIR o -DELTA 3 -MINEVIDENCE 5 -RNMIN 2 -GENETAG GE -T 4 -cageCo 10".split(),
                          "CollapseModel", cli.CM_OPTIONS, cli.CM_LONG)
    b = cli._picard_parse("INPUT=a.bam REFFLAT=r CSV=c OUTDIR=o DELTA=3 MINEVIDENCE=5 RNMIN=2 GENETAG=GE nThreads=4 cageCo=10".split(),
                          "CollapseModel", cli.CM_OPTIONS, cli.CM_LONG)
    assert a == b == dict(I="a.bam", REFFLAT="r", CSV="c", OUTDIR="o", DELTA=3, MINEVIDENCE=5, RNMIN=2, GENETAG="GE", T=4, cageCo=10)
    assert {k: d for k, (_f, _k, d) in cli.CM_OPTIONS.items() if d is not None} == dict(
        DELTA=2, MINEVIDENCE=2, RNMIN=1, PREFIX="CollapseModel", CELLTAG="BC", UMITAG="U8", GENETAG="IG", ISOFORMTAG="IT", RNTAG="RN", MAXCLIP=150,
        TSOENDTAG="TE", POLYASTARTTAG="PS", CDNATAG="CS", USTAG="US", T=20, MAXUMIS=20, MINPS=3, MAXPS=20, DEBUG=False, cageCo=50, polyaCo=50,
        juncCo=1, VALIDATION_STRINGENCY="STRICT")
    assert {k: f for k, (f, _k, _d) in cli.CM_OPTIONS.items() if f} == dict(
        DELTA="delta", MINEVIDENCE="min_evidence", RNMIN="rn_min", CELLTAG="cell_tag", UMITAG="umi_tag", GENETAG="gene_tag", ISOFORMTAG="iso_tag",
        RNTAG="rn_tag", MAXCLIP="max_clip")


def test_cli_required_options_and_the_validator_refusal(cli, tmp_path, capsys, monkeypatch):
    for k in ("i.bam", "r.refFlat", "c.csv", "cage.bed", "polya.bed", "short.bam"):
        (tmp_path / k).write_bytes(b"")
    base = [f"I={tmp_path / 'i.bam'}", f"REFFLAT={tmp_path / 'r.refFlat'}", f"CSV={tmp_path / 'c.csv'}", f"OUTDIR={tmp_path}"]
    for drop in range(4):
        assert cli.main(["CollapseModel"] + base[:drop] + base[drop + 1:]) == 1
        assert "missing required option(s) " + base[drop].split("=")[0] in capsys.readouterr().err
    assert cli.main(["CollapseModel"] + base[1:] + [f"I={tmp_path / 'nope.bam'}"]) == 1
    assert "no such file" in capsys.readouterr().err
    assert cli.main(["CollapseModel"] + base[:3] + [f"OUTDIR={tmp_path / 'nodir'}"]) == 1
    assert "no such directory" in capsys.readouterr().err
    val = [f"CAGE={tmp_path / 'cage.bed'}", f"POLYA={tmp_path / 'polya.bed'}", f"SHORT={tmp_path / 'short.bam'}"]
    assert cli.main(["CollapseModel"] + base + val) == 1
    assert "the validator is not part of this build" in capsys.readouterr().err
    assert cli.main(["CollapseModel", "-I", str(tmp_path / "i.bam"), "-REFFLAT", str(tmp_path / "r.refFlat"), "-CSV", str(tmp_path / "c.csv"),
                     "-OUTDIR", str(tmp_path), "-CAGE", val[0][5:], "-POLYA", val[1][6:], "-SHORT", val[2][6:]]) == 1
    assert "the validator is not part of this build" in capsys.readouterr().err
    # one of the three missing, or naming no file: the reference runs without validation, and so does this build
    seen = []
    cm = importlib.import_module("sicelore_amd.collapsemodel")
    monkeypatch.setattr(cli, "_context", lambda: "ctx")
    monkeypatch.setattr(cm, "collapse_model", lambda ctx, *a, **kw: seen.append((a, kw)) or dict(kept=0, records=0, genes=0, isoforms=0, gencode=0))
    assert cli.main(["CollapseModel"] + base + val[:2]) == 0
    assert cli.main(["CollapseModel"] + base + val[:2] + [f"SHORT={tmp_path / 'absent.bam'}", "MINEVIDENCE=5"]) == 0
    assert len(seen) == 2 and seen[0][1]["min_evidence"] == 2 and seen[1][1]["min_evidence"] == 5 and seen[0][1]["gene_tag"] == "IG"
    assert seen[0][1]["prefix"] == "CollapseModel" and cm.output_names("P", 2, 1, 5)[".final.gff"] == "P.d2.rn1.e5.final.gff"


def test_statistics_block(pkg, hand):
    cm = importlib.import_module("sicelore_amd.collapsemodel")
    lines = cm.statistics_lines(hand[1])
    assert lines[0] == "\tCells detected\t\t[3]" and lines[2] == "Loader Bam End...8" and lines[3] == "Collapser Start...[8 total genes]"
    assert lines[8] == "total_genes\t\t\t\t8" and lines[9] == "total_isoforms\t\t\t\t18 (37)\t3 (5)"
    assert lines[11] == " o gencode\t\t\t\t3 (5)\t3 (5)" and lines[13] == " o combination_of_known_junctions\t1 (2)\t0 (0)"
    assert lines[16] == " o at_least_one_novel_splicesite\t13 (28)\t0 (0)"


def test_exports_and_header_agree(pkg):
    import os

    lib = importlib.import_module("sicelore_amd.lib")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sicelore_mi.h")).read()
    for name in ("smi_collapse_default_config", "smi_collapse_create", "smi_collapse_set_references", "smi_collapse_add_segment", "smi_collapse_run",
                 "smi_collapse_output", "smi_collapse_counts", "smi_collapse_error_read", "smi_collapse_free", "smi_collapse_host_loop"):
        assert name in lib.EXPORTS and f"int {name}(" in hdr
    assert hdr.count("#define SMI_COL_") - 5 == len(lib.COLLAPSE_COUNTS) == 30 and len(lib.COLLAPSE_OUTPUTS) == 5
    assert set(m.COUNT_KEYS) == set(lib.COLLAPSE_COUNTS) - {"long_lists"}


# ---- the edges the GPU tests claim ------------------------------------------------------------------------------------------------------
def test_gpu_edges_are_in_their_inputs():
    bam, ref, csv = cc.sizes_case()
    _o, cnt, det = m.collapse_model(bam, ref, csv)
    assert [det[f"S{n:03d}"]["undef"] for n in (0, 1, 63, 64, 65, cc.BLOCK + 1)] == [0, 1, 63, 64, 65, cc.BLOCK + 1]
    assert all(len(det[f"S{n:03d}"]["founders"]) == 1 for n in (1, 63, 64, 65, cc.BLOCK + 1)) and cnt["max_undef"] == cc.BLOCK + 1
    bam, ref, csv = cc.founders_case()
    _o, cnt, det = m.collapse_model(bam, ref, csv)
    assert [len(det[f"F{n:03d}"]["founders"]) for n in (1, 63, 64, 65, 300)] == [1, 63, 64, 65, 300]
    assert sorted(set(c for _t, c in det["F300"]["founders"])) == [1, 2, 3] and cnt["novel_evidenced"] < cnt["founders"]
    bam, ref, csv = cc.junction_lists_case()
    _o, cnt, det = m.collapse_model(bam, ref, csv)
    assert det["JL"]["founders"] == [(f"Novel.{i}", 2) for i in range(1, 6)]
    assert [ne - 1 for _t, _s, ne in det["JL"]["kept"]] == [cc.LDS_JUNC + 1, 65, 64, 63, 1]
    bam, ref, csv = cc.filter_lists_case()
    _o, cnt, det = m.collapse_model(bam, ref, csv)
    for n in cc.FILTER_TARGETS:
        d = det[f"L{n:03d}"]
        known = [k for k in d["kept"] if k[1] == "gencode"]
        model_lines = ref.count(f"L{n:03d}\t")
        assert len(known) + model_lines == n and len(d["dropped"]) == 1 and len(d["kept"]) == len(known) + 1
    founders = {}
    for delta in (-1, 0, 2, 6000):
        bam, ref, csv = cc.seeded_case(5)
        _o, cnt, det = m.collapse_model(bam, ref, csv, delta=delta, min_evidence=1 if delta < 0 else 2)
        founders[delta] = cnt["founders"]
        assert cnt["founders"] > 0 and cnt["isoforms"] > cnt["gencode"] > 0
        if delta == -1:                          # isIn never holds: every record with a junction founds, no novel is dropped or known
            assert cnt["founders"] == cnt["undef_records"] - cnt["monoexon"] and cnt["novel_filtered"] == 0 and cnt["ckj"] == 0
        if delta == 2:
            assert cnt["ckj"] and cnt["cks"] and cnt["nss"] and cnt["novel_filtered"] and cnt["monoexon"] and cnt["low_rn"] == 0
            assert cnt["novel_evidenced"] < cnt["founders"]
        if delta == 6000:                        # a gene spans less than 6000: every list of one length of a gene joins one founder
            assert max(len(d["founders"]) for d in det.values()) <= 4
    assert founders[-1] > founders[0] > founders[2] > founders[6000]
    _o, cnt2, _d = m.collapse_model(*cc.seeded_case(5), rn_min=2)
    _o, cnt3, _d = m.collapse_model(*cc.seeded_case(5), rn_min=4)
    assert 0 < cnt2["low_rn"] < cnt2["records"] and cnt3["kept"] == 0
