"""FusionDetector without a GPU: tests/fusionmodel.py against output written out by hand for the hand-built case of
tests/fusioncases.py, the HashSet bucket rule, Java's split, the command line, the messages, and that every edge
tests/test_fusion_gpu.py claims is really in its input (asserted with the model)."""
import importlib
import os

import pytest

import fusioncases as fc
import fusionmodel as m

# by hand from the records of fusioncases.hand_records (their comments say what each is there for): cells CELL1 CELL2 CELL3
HAND_MATRIX = ("geneId\ttranscriptId\tnbExons\tCELL1\tCELL2\tCELL3\n"
               "ALK|EML4\tALK|EML4\tna\t1\t1\t0\n"          # s1, s2: a shared bucket, byte order whatever the input order
               "Aa|BB\tAa|BB\tna\t0\t0\t2\n"                # s3, s4: one hash
               "BCR|ABL1\tBCR|ABL1\tna\t1\t0\t2\n"          # r3; x1 + x2, y1 + y2
               "F1|F2\tF1|F2\tna\t0\t5\t5\n"
               "F3|F4\tF3|F4\tna\t0\t0\t10\n"
               "F6|F5\tF6|F5\tna\t0\t9\t0\n"                # F6 is in bucket 0, F5 in 15
               "GA|GB\tGA|GB\tna\t2\t2\t0\n"                # m1 and ln; rbc and m2 (nu has no UMI, ul no listed cell, t3 three genes)
               "TMPRSS2|ERG\tTMPRSS2|ERG\tna\t1\t1\t0\n"    # ab1, ab2
               "|A\t|A\tna\t1\t0\t0\n")                     # ca: the empty string is a gene name
HAND_METRICS = ("geneId\ttranscriptId\tnbExons\tnbUmis\n"
                "ALK|EML4\tALK|EML4\tna\t2\nAa|BB\tAa|BB\tna\t2\nBCR|ABL1\tBCR|ABL1\tna\t3\nF1|F2\tF1|F2\tna\t10\nF3|F4\tF3|F4\tna\t10\n"
                "F6|F5\tF6|F5\tna\t9\nGA|GB\tGA|GB\tna\t4\nTMPRSS2|ERG\tTMPRSS2|ERG\tna\t2\n|A\t|A\tna\t1\n")


def _mi(cell, umi, key, reads=1, pct="0.0"):
    return f"{cell}\t{umi}\t{reads}\t0\t{pct}\t\t{key}\t{key}\n"


HAND_MOLINFOS = (
    m.MOLINFOS_HEAD +
    _mi("CELL1", "U2", "TMPRSS2|ERG", pct="0.75") +          # df 0.25, no de
    _mi("CELL1", "UC1", "|A") +
    _mi("CELL1", "UM1", "GA|GB", reads=7) +                  # RN 7
    _mi("CELL1", "UMID", "BCR|ABL1") +                       # the UMI of the middle record; one read of three records
    _mi("CELL1", "US1", "ALK|EML4") +
    _mi("CELL1", "null", "GA|GB") +                          # the UMI whose text is null
    _mi("CELL2", "U3", "TMPRSS2|ERG") +
    "".join(_mi("CELL2", f"UA{i:02d}", "F1|F2") for i in (0, 2, 4, 6, 8)) +
    _mi("CELL2", "UB", "GA|GB") +                            # the last record's barcode, the first record's UMI
    "".join(_mi("CELL2", f"UC{i:02d}", "F6|F5") for i in range(9)) +
    _mi("CELL2", "UM2", "GA|GB", pct="0.95") +               # de 0.05 wins over df 0.5
    _mi("CELL2", "US2", "ALK|EML4") +
    "".join(_mi("CELL3", f"UA{i:02d}", "F1|F2") for i in (1, 3, 5, 7, 9)) +
    "".join(_mi("CELL3", f"UB{i:02d}", "F3|F4") for i in range(10)) +
    _mi("CELL3", "US3", "Aa|BB") + _mi("CELL3", "US4", "Aa|BB") +
    _mi("CELL3", "UX", "BCR|ABL1", reads=2, pct="0.8") +     # 1 - de of the read added last (0.2)
    _mi("CELL3", "UY", "BCR|ABL1", reads=2))
HAND_COUNTS = dict(records=65, valid=56, unvalid=9, mapqv0=2, no_gene=3, no_umi=0, chimeria=2, null=2, reads=53, reads_multi=2, molecules=51,
                   molecule_reads=53, multi_ig=47, cells=3, gene_fields=100, genes=20, counted=43, rows=9)


@pytest.fixture(scope="module")
def hand():
    return m.fusion_detector(fc.hand_bam(), fc.HAND_CSV)


@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module("sicelore_amd.cli")


def test_hand_case_against_files_written_by_hand(hand):
    out, cnt, fusions, mols = hand
    assert out["_fusmatrix.txt"].decode() == HAND_MATRIX
    assert out["_fusmetrics.txt"].decode() == HAND_METRICS
    assert out["_fusmolinfos.txt"].decode() == HAND_MOLINFOS
    assert cnt == HAND_COUNTS
    by = {(x["bc"], x["umi"]): x for x in mols}
    assert by[("CELL1", "UCLIP")]["genes"] == {"GA"} and by[("CELL1", "UP0")]["genes"] == {"GA"}      # a clip of 10000, a primary mapq 0
    assert sorted(len(x["genes"]) for x in mols if x["umi"] in ("UT3", "UC2", "UC3", "UC4")) == [0, 1, 3, 3]
    assert by[("CELL1", None)]["genes"] == {"GA", "GB"} and by[("CELLX", "UU")]["genes"] == {"GA", "GB"}
    assert len(by[("CELL1", "UMID")]["reads"][0]["records"]) == 3 and ("CELL3", "UB") not in by


def test_bucket_rule():
    assert (m.java_hash("BCR"), m.bucket("BCR")) == (65585, 0) and (m.java_hash("ABL1"), m.bucket("ABL1")) == (2002246, 8)
    assert (m.bucket("TMPRSS2"), m.bucket("ERG")) == (9, 11) and (m.bucket("GA"), m.bucket("GB")) == (10, 11)
    assert m.bucket("EML4") == m.bucket("ALK") == 0 and m.java_hash("Aa") == m.java_hash("BB") == 2112
    for a, b, key in (("BCR", "ABL1", "BCR|ABL1"), ("TMPRSS2", "ERG", "TMPRSS2|ERG"), ("GA", "GB", "GA|GB"), ("EML4", "ALK", "ALK|EML4"),
                      ("Aa", "BB", "Aa|BB"), ("", "A", "|A"), ("x[1]", "GB", "x1|GB")):
        assert m.fusion_key({a, b}) == m.fusion_key([b, a]) == key
    assert m.java_hash("x[1]") == 3663983 and m.bucket("x[1]") == 8                    # in front of GB (11); the brackets go (L84-85)
    assert m.java_hash("\xe9") == 233 and m.java_hash("TMPRSS2") == 3816716727      # bytes, 32-bit wrap-around


def test_java_split():
    assert m.java_split("A,") == ["A"] and m.java_split(",A") == ["", "A"] and m.java_split("A,,B") == ["A", "", "B"]
    assert m.java_split(",") == [] and m.java_split("A,B") == ["A", "B"] and m.java_split(",,A,,") == ["", "", "A"]


def test_cli_parses_both_syntaxes_and_defaults(cli):
    a = cli._picard_parse("-I a.bam -CSV c.csv -O out -PREFIX p".split(), "FusionDetector", cli.FD_OPTIONS, cli.FD_LONG)
    b = cli._picard_parse("INPUT=a.bam CSV=c.csv OUTPUT=out PREFIX=p".split(), "FusionDetector", cli.FD_OPTIONS, cli.FD_LONG)
    assert a == b == dict(I="a.bam", CSV="c.csv", O="out", PREFIX="p")
    assert {k: d for k, (_f, _k, d) in cli.FD_OPTIONS.items() if d is not None} == dict(PREFIX="fusion", VALIDATION_STRINGENCY="STRICT")


def test_cli_required_options_missing_file_and_directory(cli, tmp_path, capsys, monkeypatch):
    for k in ("i.bam", "c.csv"):
        (tmp_path / k).write_bytes(b"")
    base = [f"I={tmp_path / 'i.bam'}", f"CSV={tmp_path / 'c.csv'}", f"O={tmp_path}"]
    for drop in range(3):
        assert cli.main(["FusionDetector"] + base[:drop] + base[drop + 1:]) == 1
        assert "missing required option(s) " + base[drop].split("=")[0] in capsys.readouterr().err
    assert cli.main(["FusionDetector"] + base[1:] + [f"I={tmp_path / 'nope.bam'}"]) == 1
    assert f"I={tmp_path / 'nope.bam'}: no such file" in capsys.readouterr().err
    assert cli.main(["FusionDetector", base[0], base[2], f"CSV={tmp_path / 'nope.csv'}"]) == 1
    assert f"CSV={tmp_path / 'nope.csv'}: no such file" in capsys.readouterr().err
    assert cli.main(["FusionDetector"] + base[:2] + [f"O={tmp_path / 'nodir'}"]) == 1
    assert f"O={tmp_path / 'nodir'}: no such directory" in capsys.readouterr().err
    assert cli.main(["FusionDetector"] + base + ["MAXCLIP=150"]) == 1              # the constants of L63-67 are no options
    assert "unknown option 'MAXCLIP'" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert cli.main(["FusionDetector"] + base) == 1
    assert "FusionDetector runs in one process on one GPU" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    seen = []
    fd = importlib.import_module("sicelore_amd.fusiondetector")
    monkeypatch.setattr(cli, "_context", lambda: "ctx")
    monkeypatch.setattr(fd, "fusion_detector", lambda ctx, *a, **kw: seen.append((a, kw)) or dict(valid=0, records=0, molecules=0, counted=0, rows=0))
    assert cli.main(["FusionDetector"] + base) == 0
    assert cli.main(["FusionDetector", "-I", base[0][2:], "-CSV", base[1][4:], "-O", base[2][2:], "-PREFIX", "p", "-VALIDATION_STRINGENCY", "SILENT"]) == 0
    assert [kw["prefix"] for _a, kw in seen] == ["fusion", "p"] and seen[0][0] == seen[1][0] == (base[0][2:], base[1][4:], base[2][2:])
    assert fd.output_names("p") == {"_fusmatrix.txt": "p_fusmatrix.txt", "_fusmetrics.txt": "p_fusmetrics.txt", "_fusmolinfos.txt": "p_fusmolinfos.txt"}


def test_the_steps_in_front_stay_refused_by_name(cli, capsys):
    for sub in ("ExportClippedReads", "AddBamReadTags", "AddBamReadSequenceTag"):
        assert cli.main([sub, "I=a.bam"]) == 1
        err = capsys.readouterr().err
        assert f"sub-command {sub!r}" in err and "CollapseModel and FusionDetector" in err


def test_message_lines(pkg, hand):
    fd = importlib.import_module("sicelore_amd.fusiondetector")
    out, cnt, fusions, _mols = hand
    assert fd.fusions_of(out["_fusmetrics.txt"]) == fusions
    lines = fd.statistics_lines(cnt, fusions)
    assert lines == m.statistics_lines(cnt, fusions) == [
        "\tCells detected\t[3]", "\tstart...", "\tend...", "\tTotal SAMrecords\t65", "\tSAMrecords valid\t56", "\tSAMrecords unvalid\t9",
        "\tSAMrecords mapqv=0\t2", "\tSAMrecords no gene\t3", "\tSAMrecords no UMI\t0", "\tSAMrecords chimeria\t2", "\tTotal reads\t\t53",
        "\tTotal reads multiSAM\t2", "\tMoleculeDataset init start...", "\tTotal molecules\t\t51", "\tTotal molecule reads\t53",
        "\tTotal molecule multiIG\t47", "\tSetFusions\t\tstart...",
        "\t10 distincts molecules support fusion [F1|F2]", "\t10 distincts molecules support fusion [F3|F4]"]       # the tie: byte order; 9: unnamed
    assert fd.statistics_lines(cnt, [("B", 11), ("C", 10), ("A", 10), ("D", 12)])[17:] == [
        f"\t{n} distincts molecules support fusion [{k}]" for k, n in (("D", 12), ("B", 11), ("A", 10), ("C", 10))]


def test_parse_errors_name_the_read():
    tm = fc.tm
    bad = dict(int_bc=fc.rec("int_bc", "GA", bc=None, extra=tm.aux_int("BC", "C", 3)), int_u8=fc.rec("int_u8", "GA", umi=None, extra=tm.aux_int("U8", "C", 3)),
               int_ge=fc.rec("int_ge", None, flag=4, extra=tm.aux_int("GE", "C", 3)),          # the three casts come first, for an unmapped record too
               z_rn=fc.rec("z_rn", "GA", extra=tm.aux_z("RN", "2")), z_de=fc.rec("z_de", "GA", df=0.1, extra=tm.aux_z("de", "0.1")),
               z_df=fc.rec("z_df", "GA", extra=tm.aux_z("df", "0.1")), walk=fc.rec("walk", "undef", cigar=[("S", 40)]), no_cigar=fc.rec("no_cigar", "GA", cigar=[]))
    recs = fc.hand_records()
    for which, r in bad.items():
        with pytest.raises(m.FusionError) as e:
            m.fusion_detector(fc.bam(recs[:30] + [r] + recs[30:]), fc.HAND_CSV)
        assert e.value.read == which
    # not reached: RN, de and the CIGAR of a record without BC or with the unmapped flag; df behind a float de
    ok = [fc.rec("a", "GA", flag=4, cigar=[], extra=tm.aux_z("RN", "2") + tm.aux_z("de", "x")), fc.rec("b", "GA", de=0.5, extra=tm.aux_z("df", "x"))]
    assert m.fusion_detector(fc.bam(ok), fc.HAND_CSV)[1]["valid"] == 1


def test_exports_and_header_agree(pkg):
    lib = importlib.import_module("sicelore_amd.lib")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sicelore_mi.h")).read()
    for name in ("smi_fusion_default_config", "smi_fusion_create", "smi_fusion_add_segment", "smi_fusion_run", "smi_fusion_output", "smi_fusion_counts",
                 "smi_fusion_error_read", "smi_fusion_free", "smi_fusion_host_loop"):
        assert name in lib.EXPORTS and f"int {name}(" in hdr
    assert hdr.count("#define SMI_FUS_") - 3 == len(lib.FUSION_COUNTS) == 21 and lib.FUSION_OUTPUTS == m.SUFFIXES
    assert set(m.COUNT_KEYS) == set(lib.FUSION_COUNTS) - {"render_blocks", "probe_steps", "wraps"} and len(lib.FUSION_STAGES) == 6


# ---- the edges the GPU tests claim ------------------------------------------------------------------------------------------------------
def _mols(case):
    bam, csv = case
    out, cnt, fusions, mols = m.fusion_detector(bam, csv)
    return out, cnt, fusions, mols


def test_gpu_edges_are_in_their_inputs():
    out, cnt, fusions, mols = _mols(fc.read_sizes_case())
    assert sorted(len(rd["records"]) for x in mols for rd in x["reads"]) == [1, 2, 63, 64, 65]
    assert {(x["bc"], x["umi"]) for x in mols} == {("CELL1", f"U{n}") for n in (1, 2, 63, 64, 65)} and fusions == [("GA|GB", 4)]
    out, cnt, fusions, mols = _mols(fc.molecule_sizes_case())
    assert sorted(len(x["reads"]) for x in mols) == [1, 63, 64, 65, 300] and cnt["counted"] == 4
    mi = out["_fusmolinfos.txt"].decode().split("\n")
    assert "CELL0\tUM300\t300\t0\t0.701\t\tGA|GB\tGA|GB" in mi and "CELL4\tUM64\t64\t0\t0.937\t\tGA|GB\tGA|GB" in mi   # rn 1 of the first read
    out, cnt, fusions, mols = _mols(fc.gene_counts_case())
    assert sorted(len(x["genes"]) for x in mols) == [1, 2, 3, 65] and cnt["counted"] == 1 and cnt["gene_fields"] == 138
    out, cnt, fusions, mols = _mols(fc.keys_case())
    assert cnt["reads"] == 4 + 8 + 8 + 2 and cnt["reads_multi"] == 1 and {1, 200} <= {len(g) for x in mols for g in x["genes"]}
    assert [k for k, _n in fusions] == ["GA|GB", "G|GA", "G|GAB", "G|GAC", "G|Z", fc.LONG[:-1] + "M|" + fc.LONG]      # G is in bucket 7
    assert dict(fusions)[fc.LONG[:-1] + "M|" + fc.LONG] == 2 and cnt["molecules"] == 1 + 4 + 4 + 1 and cnt["counted"] == 4 + 2 + 1
    assert "CELL3:\tUQ\t2\t0\t0.0\t\tGA|GB\tGA|GB" in out["_fusmolinfos.txt"].decode().split("\n")
    out, cnt, fusions, mols = _mols(fc.tight_table_case())
    assert cnt["valid"] == cnt["reads"] == cnt["gene_fields"] == 64 and cnt["cells"] == 8 and cnt["counted"] == cnt["rows"] == 32
    out, cnt, fusions, mols = _mols(fc.none_counted_case())
    assert cnt["counted"] == 0 and out["_fusmatrix.txt"] == b"geneId\ttranscriptId\tnbExons\tCELL0\tCELL1\tCELL2\tCELL3\tCELL4\n"
    assert out["_fusmetrics.txt"].count(b"\n") == 1 and out["_fusmolinfos.txt"] == m.MOLINFOS_HEAD.encode()
    for n in (1, 63, 64, 65, 200):
        assert _mols(fc.rows_case(n))[1]["rows"] == n
    out, cnt, fusions, mols = _mols(fc.big_row_case())
    assert out["_fusmatrix.txt"].endswith(b"BCR|ABL1\tBCR|ABL1\tna\t0\t1001\t0\t0\t3\n") and fusions == [("BCR|ABL1", 1004)]
    out, cnt, fusions, mols = _mols((fc.bam([]), fc.CSV5))
    assert cnt["records"] == 0 and out["_fusmolinfos.txt"] == m.MOLINFOS_HEAD.encode()


def test_seeded_case_is_what_the_gpu_test_says():
    out, cnt, fusions, mols = _mols(fc.seeded_case(3))
    two = sum(len(x["genes"]) == 2 for x in mols)
    assert 19000 < cnt["records"] < 21000 and 2000 < cnt["molecules"] < 5000 and 0.05 < two / len(mols) < 0.2
    assert min(cnt[k] for k in ("mapqv0", "no_gene", "chimeria", "null", "reads_multi", "counted")) > 50
    assert any(x["umi"] is None for x in mols) and any(len(x["genes"]) == 3 for x in mols) and cnt["counted"] < two
