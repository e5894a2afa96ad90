"""SNPMatrix without a GPU: tests/snpmodel.py against expectations worked out by hand, and the command line."""
import importlib

import pytest

import bammodel
import snpmodel as sm

MOLHEAD = "cellBC\tUMI\tnbReads\tnbSupportingReads\tmappingPctId\tsnpPhredScore\tgeneId\ttranscriptId\n"


def test_read_position_by_hand():
    M, D, N, I, S, H = "M", "D", "N", "I", "S", "H"
    c = [(M, 50), (D, 2), (M, 50)]                        # reference 1000..1049 = read 1..50, 1050..1051 deleted, 1052..1101 = read 51..100
    assert [sm.read_position(1000, c, p) for p in (999, 1000, 1010, 1049, 1050, 1051, 1052, 1060, 1101, 1102)] == [0, 1, 11, 50, 0, 0, 51, 59, 100, 0]
    assert sm.read_position(2000, [(S, 5), (M, 95)], 2000) == 6      # S counts in the read offset
    assert sm.read_position(3000, [(H, 5), (M, 100)], 3000) == 1     # H does not
    c = [(M, 10), (I, 3), (M, 87)]
    assert [sm.read_position(4000, c, p) for p in (4009, 4010)] == [10, 14]
    c = [(M, 20), (N, 500), (M, 80)]
    assert [sm.read_position(5000, c, p) for p in (5019, 5020, 5100, 5519, 5520)] == [20, 0, 0, 0, 21]
    assert sm.reference_length(c) == 600


def test_hand_built_case_against_hand_worked_files():
    """bases are "ACGT"[i % 4] and qualities i % 40 + 2 at read index i, so every expected line below is arithmetic:
    fwd_del 50M2D50M at 1000: 1010 -> read 11 (index 10: G, 12); 1050 in the deletion; 1060 -> read 59 (index 58: G, 20); 1101 -> read 100
    = the read length, rejected by the strict >.  clip 5S95M at 2000 -> read 6 (C, 7).  hclip 5H100M at 3000 -> read 1 (A, 2), RN 5.
    ins 10M3I87M at 4000: 4010 -> read 14 (C, 15).  gap 20M500N80M at 5000: 5100 in the intron, 5520 -> read 21 (A, 22).
    rev_n (reverse, N at index 10): 6010, 6011 -> N -> "", T -> A, qualities 12,13.  fwd_n keeps its N.  two (400M at 7000, twice, one
    secondary): the line says 7302|7101, bases come for 7101 (index 101: C, 23) then 7302 (index 302: G, 24)."""
    out, cnt, per_line = sm.snp_matrix(sm.hand_bam(), sm.SNP, sm.CSV)
    rows = [("after\tchr1:1060..G", "1\t0\t0\t0"), ("afterN\tchr1:5520..A", "1\t0\t0\t0"), ("before\tchr1:1010..G", "1\t0\t0\t0"),
            ("chr2site\tchr2:1010..G", "0\t1\t0\t0"), ("clipH\tchr1:3000..A", "0\t1\t0\t0"), ("clipS\tchr1:2000..C", "0\t1\t0\t0"),
            ("fwdN\tchr1:6010..N", "0\t0\t1\t0"), ("ins\tchr1:4010..C", "1\t0\t0\t0"), ("revN\tchr1:6010|6011..A", "0\t0\t1\t0"),
            ("swapped\tchr1:7302|7101..CG", "1\t0\t0\t0")]
    assert out["snpmatrix.txt"].decode() == ("geneId\ttranscriptId\tnbExons\tCELL1\tCELL2\tCELL3\tCELL4\n"
                                             + "".join(f"{k}\tna\t{v}\n" for k, v in rows))
    assert out["snpmetrics.txt"].decode() == "geneId\ttranscriptId\tnbExons\tnbUmis\n" + "".join(f"{k}\tna\t1\n" for k, _v in rows)
    assert out["snpmolinfos.txt"].decode() == MOLHEAD + (
        "CELL1\tUMI1\t1\t0\tnull\t12\tbefore\tchr1:1010..G\n"
        "CELL1\tUMI1\t1\t0\tnull\t20\tafter\tchr1:1060..G\n"
        "CELL2\tUMI2\t1\t0\tnull\t7\tclipS\tchr1:2000..C\n"
        "CELL2\tUMI3\t5\t0\tnull\t2\tclipH\tchr1:3000..A\n"
        "CELL1\tUMI1\t1\t0\tnull\t15\tins\tchr1:4010..C\n"
        "CELL1\tUMI4\t1\t0\tnull\t22\tafterN\tchr1:5520..A\n"
        "CELL3\tUMI5\t1\t0\tnull\t12,13\trevN\tchr1:6010|6011..A\n"
        "CELL3\tUMI6\t1\t0\tnull\t12\tfwdN\tchr1:6010..N\n"
        "CELL1\tUMI7\t1\t0\tnull\t23,24\tswapped\tchr1:7302|7101..CG\n"       # the same (cell, UMI) twice: two lines, one count
        "CELL1\tUMI7\t1\t0\tnull\t23,24\tswapped\tchr1:7302|7101..CG\n"
        "CELL2\tUMI9\t1\t0\tnull\t12\tchr2site\tchr2:1010..G\n")
    # the header line and chrZ are not in the dictionary; the line behind the blank one is never read; the CELLX hit on clipS counts
    assert [(c["line"].split(",")[3], c["hits"]) for c in per_line] == [
        ("before", 1), ("indel", 0), ("after", 1), ("lastbase", 0), ("clipS", 2), ("clipH", 1), ("ins", 1), ("inN", 0), ("afterN", 1),
        ("revN", 1), ("fwdN", 1), ("swapped", 2), ("chr2site", 1)]
    assert cnt == dict(records=13, lines=13, cells=4, hits=12, lowRN=0, lowQV=0, pairs=12, kept=11, rows=10, total_count=10)


def test_minrn_and_minqv_by_hand():
    out, cnt, _ = sm.snp_matrix(sm.hand_bam(), sm.SNP, sm.CSV, min_rn=2)      # only hclip has RN 5; absent and 1 are below 2
    assert (cnt["hits"], cnt["lowRN"], cnt["lowQV"], cnt["rows"]) == (1, 11, 0, 1)
    assert out["snpmolinfos.txt"].decode() == MOLHEAD + "CELL2\tUMI3\t5\t0\tnull\t2\tclipH\tchr1:3000..A\n"
    out, cnt, _ = sm.snp_matrix(sm.hand_bam(), sm.SNP, sm.CSV, min_qv=13)     # qualities 12, 7 (twice), 2, 12 (revN's smaller), 12, 12 fall below 13
    assert (cnt["hits"], cnt["lowRN"], cnt["lowQV"]) == (5, 0, 7)
    assert sorted(k.split(b"\t")[0] for k in out["snpmetrics.txt"].split(b"\n")[1:-1]) == [b"after", b"afterN", b"ins", b"swapped"]
    _o, cnt, _ = sm.snp_matrix(sm.hand_bam(), sm.SNP, sm.CSV, min_qv=101)     # min_qv starts at 100
    assert (cnt["hits"], cnt["lowQV"]) == (0, 12)


def test_empty_result_writes_no_file():
    out, cnt, per_line = sm.snp_matrix(sm.hand_bam(), "chr1,900000,+,far\n", sm.CSV)
    assert out == {} and cnt["rows"] == 0 and cnt["hits"] == 0 and len(per_line) == 1
    out, cnt, _ = sm.snp_matrix(sm.hand_bam(), "chr1,2000,+,clipS\n", "CELL9\n")   # hits, but of no listed cell
    assert out == {} and cnt["hits"] == 2 and cnt["kept"] == 0


def test_snp_file_rules():
    names = ["chr1", "chr2"]
    kept = sm.parse_snp("x,y\nchr1,300|100,-,g\r\nchr2,7,+,h,extra\n\nchr1,1,+,never\n", names)
    assert [(k["chrom"], k["pos"], k["arr"], k["neg"], k["gene"]) for k in kept] == [("chr1", ["300", "100"], [100, 300], True, "g"),
                                                                                   ("chr2", ["7"], [7], False, "h")]
    assert sm.parse_snp("chr1,100|,+,g\n", names)[0]["pos"] == ["100"]            # split drops the trailing empty string
    for bad, msg in (("chr1,12x,+,g\n", "not an integer"), ("chr1,5,+\n", "4 are needed"), ("chr1,|,+,g\n", "no position")):
        with pytest.raises(sm.SnpError, match=msg):
            sm.parse_snp(bad, names)
    assert sm.parse_snp("chrZ,12x\n", names) == []                                # an unknown chromosome is skipped before anything is parsed


def test_record_errors_name_the_read():
    import tagbammodel as tm

    def run(r, snp="chr1,1010,+,s\n"):
        return sm.snp_matrix(bammodel.bam_bytes(sm.HEAD, sm.REFS, [r]), snp, sm.CSV)
    with pytest.raises(sm.SnpError, match="read noq: no base qualities"):
        run(sm.rec("noq", [("M", 100)], 1000, "CELL1", "U", qual=b"\xff" * 100))
    with pytest.raises(sm.SnpError, match="read noumi: a hit of cell CELL1 without the UMI"):
        run(sm.rec("noumi", [("M", 100)], 1000, "CELL1", None))
    assert run(sm.rec("noumi", [("M", 100)], 1000, "CELLX", None))[1]["hits"] == 1          # not kept: no UMI is needed
    with pytest.raises(sm.SnpError, match="read badrn: attribute RN"):
        run(sm.rec("badrn", [("M", 100)], 1000, "CELL1", "U", extra=tm.aux_z("RN", "5")))
    with pytest.raises(sm.SnpError, match="read walk: the CIGAR walk"):
        run(sm.rec("walk", [("M", 100), ("D", 10), ("H", 5)], 1000, "CELL1", "U"))
    assert run(sm.rec("far", [("M", 100), ("D", 10), ("H", 5)], 50000, "CELL1", "U"))[1]["hits"] == 0   # never queried


@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module("sicelore_amd.cli")


def test_cli_missing_options_and_files(cli, capsys, tmp_path):
    assert cli.main(["SNPMatrix", "I=x.bam", "CSV=c.csv", "O=."]) == 1
    assert "missing required option(s) SNP" in capsys.readouterr().err
    for n in ("c.csv", "s.csv"):
        (tmp_path / n).write_text("x\n")
    assert cli.main(["SNPMatrix", f"INPUT={tmp_path / 'nope.bam'}", f"CSV={tmp_path / 'c.csv'}", f"SNP={tmp_path / 's.csv'}", f"OUTPUT={tmp_path}"]) == 1
    err = capsys.readouterr().err
    assert f"I={tmp_path / 'nope.bam'}: no such file" in err                        # INPUT= / OUTPUT= parsed as I / O
    (tmp_path / "in.bam").write_bytes(b"x")
    assert cli.main(["SNPMatrix", "-I", str(tmp_path / "in.bam"), "-CSV", str(tmp_path / "c.csv"), "-SNP", str(tmp_path / "gone.csv"), "-O", str(tmp_path)]) == 1
    assert f"SNP={tmp_path / 'gone.csv'}: no such file" in capsys.readouterr().err
    assert cli.main(["SNPMatrix", "I=a", "CSV=b", "SNP=c", "O=d", "MINHITS=3"]) == 1
    assert "unknown option 'MINHITS'" in capsys.readouterr().err
    assert cli.main(["Nonsense"]) == 1
    assert "SNPMatrix" in capsys.readouterr().err                                   # listed among what is built
