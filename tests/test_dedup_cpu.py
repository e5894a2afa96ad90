"""DeduplicateMolecule without a GPU: tests/dedupmodel.py against outputs written out by hand, and the command line."""
import importlib

import pytest

import dedupmodel as dm

# HAND_FASTQ with SELECT: one record per molecule, in the input order of the winners.  A-U1: rn 2 beats rn 1 and the text of its '+' line
# goes.  N-U9 (sequence `null`) is absent.  ABC: equal rn, the longer sequence.  007 and +7 come out as 7.  T1: rn 5 beats rn 4 whatever the
# length, 5 bases beat 3, and of the two with 5 bases the first stays.
HAND_FASTQ_SELECT = (
    b"@A-U1-2\nACGTA\n+\nIIIII\n"
    b"@B-U2-3\nAC\n+\nII\n"
    b"@C-U3-4\nACG\n+\nII\n"
    b"@D-U4-5\nA\n+\nI\n"
    b"@E|x-U5-6\nAC\n+\nII\n"
    b"@F-U6-7\nACGT\n+\nIIII\n"
    b"@-U7-8\nAC\n+\nII\n"
    b"@G-U8-9\nACG\n+\nIII\n"
    b"@H-U9-10\nACGT\n+\nIIII\n"
    b"@A-BC-1\nAAAA\n+\nIIII\n"
    b"@Z-R0-0\nA\n+\nI\n@Z-R1-7\nA\n+\nI\n@Z-R2-7\nA\n+\nI\n@Z-R3-2147483647\nA\n+\nI\n"
    b"@T-1-5\nGGGGG\n+\nIIIII\n"
    b"@W-1-2\nAC\n+\nII\n")
# SELECT=false: the first record of every molecule
HAND_FASTQ_FIRST = (HAND_FASTQ_SELECT.replace(b"@A-U1-2\nACGTA\n+\nIIIII\n", b"@A-U1-1\nACGT\n+\n@III\n")
                    .replace(b"@A-BC-1\nAAAA\n+\nIIII\n", b"@AB-C-1\nAAA\n+\nIII\n").replace(b"@T-1-5\nGGGGG\n+\nIIIII\n", b"@T-1-5\nCCC\n+\nIII\n"))
# HAND_FASTA: M: the last non-empty record of rn 3; P: two empty ones, the first; Q: rn 2 wins though its sequence is empty
HAND_FASTA_OUT = b">M-1-3\nCCC\n>P-1-1\n\n>Q-1-2\n\n>R-1-4\nACGT\n"


def test_hand_fastq_select():
    out, cnt = dm.dedup(dm.HAND_FASTQ)
    assert out == HAND_FASTQ_SELECT
    # 91 lines: 1 in front, 2 stray, 21 records of 4 and the `null` record's 4 -- the last line has no LF
    assert cnt == dict(lines=91, records=21, null_records=1, skipped_lines=3, molecules=16, bytes_written=len(HAND_FASTQ_SELECT))


def test_hand_fastq_first():
    out, cnt = dm.dedup(dm.HAND_FASTQ, select=False)
    assert out == HAND_FASTQ_FIRST
    assert (cnt["records"], cnt["molecules"]) == (21, 16)


def test_hand_fasta():
    out, cnt = dm.dedup(dm.HAND_FASTA, fasta=True)
    assert out == HAND_FASTA_OUT
    assert dm.dedup(dm.HAND_FASTA, fasta=True, select=False)[0] == HAND_FASTA_OUT        # SELECT is a FASTQ option (L46-53)
    assert cnt == dict(lines=23, records=10, null_records=1, skipped_lines=1, molecules=4, bytes_written=len(HAND_FASTA_OUT))


def test_reader_by_hand():
    # a quality line that starts with '@' starts nothing; a junk line costs only itself; four '@' lines are one record
    recs, cnt = dm.read_records(b"x\n@a-b-1\n@c-d-2\n@e-f-3\n@g-h-4\ny\n\n@i-j-5\nAC\n+\nII\n")
    assert [(r["line"], r["key"], r["seq"], r["qual"]) for r in recs] == [(2, b"ab", b"@c-d-2", b"@g-h-4"), (8, b"ij", b"AC", b"II")]
    assert cnt == dict(lines=11, records=2, null_records=0, skipped_lines=3)
    # FASTA: a '>' line behind a header is its sequence
    recs, cnt = dm.read_records(b">a-b-1\n>c-d-2\nAC\n>e-f-3\nGG\n", fasta=True)
    assert [(r["line"], r["key"], r["seq"]) for r in recs] == [(1, b"ab", b">c-d-2"), (4, b"ef", b"GG")]
    assert cnt["skipped_lines"] == 1
    assert dm.dedup(b"") == (b"", dict(lines=0, records=0, null_records=0, skipped_lines=0, molecules=0, bytes_written=0))
    assert dm.dedup(b"no record\n\n+\n")[1]["skipped_lines"] == 3


def test_line_ends_by_hand():
    assert dm.split_lines(b"a\r\nb\rc\r\r\n\nd") == [(0, b"a"), (3, b"b\rc\r"), (9, b""), (10, b"d")]    # one CR in front of the LF, no other
    assert dm.split_lines(b"a\n") == [(0, b"a")] and dm.split_lines(b"") == []
    assert dm.dedup(b"@a-b-1\r\nA\rC\r\n+\r\nIII\r\n")[0] == b"@a-b-1\nA\rC\n+\nIII\n"
    assert dm.dedup(b"@a-b-1\nnull\r\n+\nIII\n")[1]["null_records"] == 1
    assert dm.dedup(b"@a-b-1\nnull \n+\nIII\n")[1]["null_records"] == 0
    assert dm.dedup(b"@a-b-1\nnull")[1] == dict(lines=2, records=0, null_records=1, skipped_lines=0, molecules=0, bytes_written=0)


def test_name_rules_by_hand():
    assert dm.normalise(b"@@C@-U3-4", b"@") == b"C-U3-4"
    assert dm.normalise(b"@F\\@|U6\\@|7", b"@") == b"F-U6-7"
    assert dm.normalise(b"@a\\\\|b|c\\d", b"@") == b"a\\-b|c\\d"
    assert dm.java_split(b"-U7-8") == [b"", b"U7", b"8"]
    assert dm.java_split(b"G-U8-9--") == [b"G", b"U8", b"9"]
    assert dm.java_split(b"---") == [] and dm.java_split(b"") == [b""] and dm.java_split(b"a--b") == [b"a", b"", b"b"]
    assert [dm.java_int(x) for x in (b"0", b"007", b"+7", b"2147483647", b"2147483648", b"", b"+", b" 7", b"7 ", b"1e3", b"0000000000000000000012")] == [
        0, 7, 7, 2147483647, None, None, None, None, None, None, 12]
    assert dm.fnv1a(b"") == 0xcbf29ce484222325 and dm.fnv1a(b"a") == 0xaf63dc4c8601ec8c        # the published FNV-1a test vectors
    # an empty key is a key
    assert dm.dedup(b"@--3\nA\n+\nI\n@--4\nC\n+\nI\n")[0] == b"@--4\nC\n+\nI\n"


def test_tie_rules_by_hand():
    fq = lambda *rs: b"".join(b"@k-u-%d\n%s\n+\n%s\n" % (rn, s, b"I" * len(s)) for rn, s in rs)   # noqa: E731
    assert dm.dedup(fq((1, b"AAAA"), (2, b"C"), (2, b"GG"), (2, b"TT"), (1, b"AAAAAAAA")))[0] == fq((2, b"GG"))
    assert dm.dedup(fq((1, b"AAAA"), (2, b"C"), (2, b"GG")), select=False)[0] == fq((1, b"AAAA"))
    assert dm.dedup(fq((3, b""), (3, b"")))[0] == fq((3, b""))
    fa = lambda *rs: b"".join(b">k-u-%d\n%s\n" % (rn, s) for rn, s in rs)                      # noqa: E731
    assert dm.dedup(fa((2, b"AAAA"), (2, b"C"), (2, b""), (1, b"GGGGGGGG")), fasta=True)[0] == fa((2, b"C"))
    assert dm.dedup(fa((2, b""), (2, b""), (1, b"G")), fasta=True)[0] == fa((2, b""))
    assert dm.dedup(fa((1, b"G"), (2, b""), (2, b"A"), (2, b"")), fasta=True)[0] == fa((2, b"A"))


@pytest.mark.parametrize("name", sorted(dm.ERROR_CASES))
def test_errors_name_the_line(name):
    data, fasta, line = dm.ERROR_CASES[name]
    for select in (True, False):
        with pytest.raises(dm.DedupError) as e:
            dm.dedup(data, fasta=fasta, select=select)
        assert e.value.line == line


@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module("sicelore_amd.cli")


def test_cli_options(cli):
    o = cli._picard_parse(["-I", "x.fq", "-O", "y.fq", "-SELECT", "true", "-VALIDATION_STRINGENCY", "SILENT"], "DeduplicateMolecule", cli.DD_OPTIONS,
                          cli.DD_LONG)
    assert o == {"I": "x.fq", "O": "y.fq", "SELECT": True, "VALIDATION_STRINGENCY": "SILENT"}
    o = cli._picard_parse(["INPUT=a.fa", "OUTPUT=b.fa", "SELECT=false", "TSO=ACGT", "MAXPOS=50"], "DeduplicateMolecule", cli.DD_OPTIONS, cli.DD_LONG)
    assert o == {"I": "a.fa", "O": "b.fa", "SELECT": False, "TSO": "ACGT", "MAXPOS": 50}


def test_cli_refusals(cli, capsys, tmp_path, monkeypatch):
    assert cli.main(["DeduplicateMolecule", f"I={tmp_path / 'nope.fq'}", f"O={tmp_path / 'out.fq'}"]) == 1
    assert f"DeduplicateMolecule: I={tmp_path / 'nope.fq'}: no such file" in capsys.readouterr().err     # (the parent answered "this build has ...")
    assert cli.main(["DeduplicateMolecule", "-O", "y.fq"]) == 1
    assert "sub-command DeduplicateMolecule: missing required option(s) I" in capsys.readouterr().err
    assert cli.main(["DeduplicateMolecule", "I=x.fq", "O=y.fq", "SELECT=maybe"]) == 1
    assert "SELECT takes true or false" in capsys.readouterr().err
    assert cli.main(["DeduplicateMolecule", "I=x.fq", "O=y.fq", "MINRN=1"]) == 1
    assert "unknown option 'MINRN'" in capsys.readouterr().err
    gz = tmp_path / "molecules.fastq.GZ"
    gz.write_bytes(b"\x1f\x8b")
    assert cli.main(["DeduplicateMolecule", f"I={gz}", f"O={tmp_path / 'out.fq'}"]) == 1
    assert ".gz input is not read" in capsys.readouterr().err
    fq = tmp_path / "in.fq"
    fq.write_bytes(dm.HAND_FASTQ)
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert cli.main(["DeduplicateMolecule", f"I={fq}", f"O={tmp_path / 'out.fq'}"]) == 1
    assert "start it without torchrun" in capsys.readouterr().err
    assert not (tmp_path / "out.fq").exists()
    assert cli.main(["Nonsense"]) == 1
    assert "DeduplicateMolecule" in capsys.readouterr().err                         # listed among what is built


def test_routing_by_file_name(pkg):
    dd = importlib.import_module("sicelore_amd.dedupmolecule")
    assert [dd.is_fastq(n) for n in ("a.fq", "/x/B.FASTQ", "c.fastq.txt", "d.fa", "fq", "e.fq.gz")] == [True, True, False, False, False, False]
    info = dict(records=5, molecules=3)
    assert dd.reference_log(info, False, True)[2:5] == ["loadFastQ\t5 sequences loaded", "loadFastQ tso\t0", "loadFastQ\t3 molecules"]
    assert dd.reference_log(info, True, True)[0] == "loadFasta\tSTART..." and dd.reference_log(info, False, False)[0] == "load/write FastQ\tSTART..."
