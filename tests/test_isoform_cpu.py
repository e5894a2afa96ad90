"""IsoformMatrix without a GPU: the reference's CIGAR walk on hand-computed cases, the refFlat parse, the cell list, Float.toString, the
writeBulk layout and the command line's errors (METHOD other than STRICT: exit 0, nothing written)."""
import importlib
import os

import pytest

import bammodel
import isoformmodel as im
import tagbammodel as tm


@pytest.mark.parametrize("cigar,want", [
    ([("M", 10), ("N", 5), ("M", 10)], [(109, 115)]),
    ([("M", 10), ("D", 21), ("M", 10)], [(109, 131)]),                      # D > 20: a short intron
    ([("M", 10), ("D", 20), ("M", 10)], []),                                # D <= 20: a deletion, e is not moved
    ([("M", 10), ("D", 30), ("N", 5), ("M", 10)], [(109, 145), (109, 145)]),  # D > 20 then N: the same junction twice
    ([("H", 5), ("S", 3), ("M", 10), ("N", 5), ("M", 10), ("S", 4), ("H", 2)], [(109, 115)]),
    ([("M", 10), ("I", 2), ("M", 8), ("N", 5), ("M", 10)], [(117, 123)]),   # I inside an exon: a block of its own
    ([("M", 10), ("N", 5), ("M", 10), ("N", 5)], [(109, 115)]),             # the last operation is never looked at
    ([("M", 10), ("N", 5)], []),
])
def test_cigar_walk(cigar, want):
    assert im.junctions(100, cigar) == want


def test_cigar_walk_without_a_block_throws():
    with pytest.raises(im.IsoformError):
        im.junctions(100, [("S", 10)])


REF = ("G1\tT1\tchr1\t+\t0\t0\t0\t0\t2\t99,199,\t110,210,\n"
       "G1\tT0\tchr1\t+\t0\t0\t0\t0\t1\t5,\t5,\n"               # zero exon bases: dropped
       "G1\tT1\tchr1\t+\t0\t0\t0\t0\t3\t99,199,299,\t110,210,310,\n"
       "G2\tT9\tchr1\t-\t0\t0\t0\t0\t1\t10,\t20,\n")


def test_refflat_parse_drop_duplicates_and_select_last():
    genes, by_gene, n = im.parse_refflat(REF)
    assert genes == ["G1", "G2"] and n == 3
    assert [t for t, _j, _n in by_gene["G1"]] == ["T1", "T1"]
    assert by_gene["G1"][0][1] == [(110, 200)]
    assert im.select(by_gene, "G1", "T1") == 3 and im.select(by_gene, "G1", "T0") == 0 and im.select(by_gene, "G3", "T1") == 0


def test_refflat_short_line_is_an_error():
    with pytest.raises(im.IsoformError, match="line 2"):
        im.parse_refflat(REF[:REF.index("\n") + 1] + "G1\tT1\tchr1\n")


def test_cell_list_minus_one_rule():
    assert im.cell_list("AAA-1\nAAA\nB-1-1C\nAAA-1\n") == ["AAA", "BC"]


@pytest.mark.parametrize("x,want", [(0.9, "0.9"), (1.0, "1.0"), (1e-4, "1.0E-4"), (-0.5, "-0.5"), (0.999, "0.999"), (1e7, "1.0E7"),
                                    (0.001, "0.001"), (123.25, "123.25"), (0.0, "0.0")])
def test_java_float_to_string(x, want):
    assert im.java_float(x) == want


HEAD = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:100000\n"


def _bam(recs):
    return bammodel.bam_bytes(HEAD, [("chr1", 100000)], recs)


def _rec(name, cigar, pos=98, bc="AAA-1", umi="U1", gene="G1"):
    aux = tm.aux_z("BC", bc) + tm.aux_z("U8", umi) + (tm.aux_z("GE", gene) if gene is not None else b"")
    return bammodel.bam_record(name, 0, 0, pos, 60, cigar, "ACGT", aux=aux)


def test_write_bulk_layout():
    bam = _bam([_rec("r1", [("M", 12), ("N", 89), ("M", 12)]), _rec("r2", [("M", 4)], umi="U2", gene="G2", pos=9)])
    out, cnt = im.isoform_matrix(bam, REF, "AAA\n", to_bulk=True)
    assert out["bulkiso.txt"] == b"transcriptId\texons\tcount\nG1\tT1\t3\t1\nG2\tT9\t1\t1\n"
    # writeBulk's second loop writes gene\ttx\tnbExons into the bulkgene stream too, without a newline
    assert out["bulkgene.txt"] == b"geneId\tcount\nG1\t1\nG2\t1\nG1\tT1\t3G2\tT9\t1"
    assert cnt["monoexon"] == 1 and cnt["onematch"] == 1


def test_model_gene_mandatory_counter():
    bam = _bam([_rec("a", [("M", 4)], gene=None), _rec("b", [("M", 4)], gene="undef"), _rec("c", [("M", 4)], gene="")])
    _out, cnt = im.isoform_matrix(bam, REF, "AAA\n")
    assert cnt["no_gene"] == 3 and cnt["valid"] == 0


@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module("sicelore_amd.cli")


def test_cli_method_other_than_strict_writes_nothing(cli, tmp_path):
    for n, t in (("in.bam", b"x"), ("r.refFlat", REF.encode()), ("c.csv", b"AAA\n")):
        (tmp_path / n).write_bytes(t)
    out = tmp_path / "out"
    out.mkdir()
    assert cli.main(["IsoformMatrix", f"I={tmp_path / 'in.bam'}", f"REFFLAT={tmp_path / 'r.refFlat'}", f"CSV={tmp_path / 'c.csv'}",
                     f"OUTDIR={out}", "METHOD=SCORE"]) == 0
    assert os.listdir(out) == []


@pytest.mark.parametrize("argv,msg", [
    (["-I", "x.bam"], "missing required option"),
    (["-I", "x.bam", "-REFFLAT", "r", "-CSV", "c", "-OUTDIR", "o", "-NOPE", "1"], "unknown option 'NOPE'"),
    (["-I", "x.bam", "-REFFLAT", "r", "-CSV", "c", "-OUTDIR", "o", "-DELTA", "two"], "DELTA 'two' is not a number"),
    (["-I", "x.bam", "-REFFLAT", "r", "-CSV", "c", "-OUTDIR", "o", "-MAPQV0", "maybe"], "MAPQV0 takes true or false"),
    (["-I", "x.bam", "-REFFLAT", "r", "-CSV", "c", "-OUTDIR", "o", "-CELLTAG", "ABC"], "not a two-character tag"),
    (["I=x.bam", "REFFLAT=r", "CSV=c", "OUTDIR=o", "VALIDATION_STRINGENCY=SILENT"], "no such file"),
])
def test_cli_errors(cli, capsys, argv, msg):
    assert cli.main(["IsoformMatrix"] + argv) == 1
    assert msg in capsys.readouterr().err
