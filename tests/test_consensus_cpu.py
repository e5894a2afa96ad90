"""ComputeConsensus without a GPU: the model's QV formula, the 1- and 2-read rules, every record filter and cDNA rule of
LongreadRecord.fromSAMRecord / LongreadParser on small BAMs, POA properties that do not depend on spoa, and the command line's errors."""
import importlib

import numpy as np
import pytest

import bammodel
import consensusmodel as cm
import tagbammodel as tm

HEAD = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:100000\n"
REFS = [("chr1", 100000)]


def rec(name, aux, flag=0, mapq=60, cigar=None, ref=0, pos=10):
    return bammodel.bam_record(name, flag, ref, pos, mapq, cigar or [("M", 4)], "ACGT", aux=aux)


def tags(bc="AAAA-1", umi="CCCC", us=None, cs=None, te=None, ps=None, de=None, df=None):
    a = b""
    if bc is not None:
        a += tm.aux_z("BC", bc)
    if umi is not None:
        a += tm.aux_z("U8", umi)
    if us is not None:
        a += tm.aux_z("US", us)
    if cs is not None:
        a += tm.aux_z("CS", cs)
    if te is not None:
        a += tm.aux_int("TE", "i", te)
    if ps is not None:
        a += tm.aux_int("PS", "S", ps)
    if de is not None:
        a += tm.aux_f("de", de)
    if df is not None:
        a += tm.aux_f("df", df)
    return a


def run(records, **kw):
    return cm.compute_consensus(bammodel.bam_bytes(HEAD, REFS, records), **kw)


def fastq_records(fq):
    lines = fq.split(b"\n")
    return [tuple(lines[i:i + 4]) for i in range(0, len(lines) - 1, 4)]


@pytest.mark.parametrize("same,rows,want", [(4, 5, 33 + 7), (5, 5, 33 + 20), (1, 3, 33 + 2), (2, 3, 33 + 5), (0, 3, 33), (19, 20, 33 + 13),
                                            (9, 10, 33 + 10), (3, 4, 33 + 6)])
def test_qv_formula(same, rows, want):
    assert cm.qv_byte(same, rows, 20) == want


def test_one_and_two_read_rules():
    assert cm.molecule_consensus([b"ACGT"], 3, 20) == (b"ACGT", b"$$$$")
    assert cm.molecule_consensus([b"ACGTA", b"ACG"], 3, 20) == (b"ACGTA", b"$$$$$")      # s1 longer
    assert cm.molecule_consensus([b"ACG", b"ACGTA"], 5, 20) == (b"ACGTA", b"&&&&&")      # s2 longer
    assert cm.molecule_consensus([b"AAAA", b"CCCC"], 3, 20) == (b"CCCC", b"$$$$")       # equal lengths: s2


def test_cdna_slicing_rules():
    us = "TTTTACGTACGTAAAAGG"          # len 18
    recs = [
        rec("r1", tags(umi="U1", us=us, te=4, ps=12)),          # US[4:12]
        rec("r2", tags(umi="U2", us=us, te=4, ps=17)),          # PS >= len-1 -> end = len-1
        rec("r3", tags(umi="U3", us=us, te=4, ps=16)),          # PS = len-2 < len-1 -> end 16
        rec("r4", tags(umi="U4", us=us, te=12, ps=12)),         # TE >= end -> the whole US
        rec("r5", tags(umi="U5", us=us)),                       # TE 0, PS 0 -> US[0:len-1]
        rec("r6", tags(umi="U6", us=us, cs="GGGG", te=4)),      # CS wins
        rec("r7", tags(umi="U7", us="", te=0)),                 # empty US: end -1 -> the whole (empty) US
    ]
    fq, cnt = run(recs)
    got = {r[0]: r[1] for r in fastq_records(fq)}
    assert got == {b"@AAAA-U1-1": b"ACGTACGT", b"@AAAA-U2-1": us[4:17].encode(), b"@AAAA-U3-1": us[4:16].encode(), b"@AAAA-U4-1": us.encode(),
                   b"@AAAA-U5-1": us[:17].encode(), b"@AAAA-U6-1": b"GGGG", b"@AAAA-U7-1": b""}
    assert cnt["valid"] == 7 and cnt["molecules"] == 7


def test_filters_and_counts():
    recs = [
        rec("nobc", tags(bc=None, us="ACGTACGT")),                                # null
        rec("unmapped", tags(us="ACGTACGT"), flag=4),                             # null
        rec("chimS", tags(us="ACGTACGT"), cigar=[("S", 151), ("M", 4)]),          # first op S > 150
        rec("chimH", tags(us="ACGTACGT"), cigar=[("M", 4), ("H", 151)]),          # last op H > 150
        rec("clip150", tags(umi="K1", us="ACGTACGT"), cigar=[("H", 150), ("M", 4), ("S", 150)]),  # not chimeric
        rec("midclip", tags(umi="K2", us="ACGTACGT"), cigar=[("M", 2), ("S", 500), ("M", 2)]),    # only the ends count
        rec("noumi", tags(umi=None, us="ACGTACGT")),
        rec("sec0", tags(umi="K3", us="ACGTACGT"), flag=256, mapq=0),             # mapq 0 secondary
        rec("sup0", tags(umi="K3", us="ACGTACGT"), flag=2048, mapq=0),            # mapq 0 supplementary
        rec("prim0", tags(umi="K4", us="ACGTACGT"), flag=0, mapq=0),              # mapq 0 primary: kept
        rec("nogene", tags(umi="K5", us="ACGTACGT")),                             # no gene tag: kept
    ]
    fq, cnt = run(recs)
    assert cnt == dict(records=11, valid=4, unvalid=7, mapqv0=2, no_gene=0, no_umi=1, chimeria=2, null=2, reads=4, reads_multi=0, molecules=4)
    names = [r[0] for r in fastq_records(fq)]
    assert names == [b"@AAAA-K1-1", b"@AAAA-K2-1", b"@AAAA-K4-1", b"@AAAA-K5-1"]
    fq, cnt = run(recs, mapqv0=True)
    assert cnt["mapqv0"] == 0 and cnt["valid"] == 6
    assert [r[0] for r in fastq_records(fq)][2] == b"@AAAA-K3-2"
    fq, cnt = run(recs, max_clip=151)
    assert cnt["chimeria"] == 0


def test_barcode_minus_one_removed_everywhere():
    fq, _ = run([rec("r", tags(bc="AC-1GT-1-1", umi="U", us="ACGTACGT"))])
    assert fq.startswith(b"@ACGT-U-1\n")


def test_de_df_and_multi_record_reads():
    recs = [
        rec("a", tags(umi="M", us="AAAAAAAAA", de=0.2)),                 # read a: records de 0.2, 0.1 (df ignored when de present)
        rec("a", tags(umi="M", us="CCCCCCCCC", de=0.1, df=0.0), flag=256),
        rec("b", tags(umi="M", us="GGGGGGGGG", df=0.05)),                # df when de is missing
        rec("c", tags(umi="M", us="TTTTTTTTTT")),                        # neither: 1.0
    ]
    fq, cnt = run(recs, max_reads=2)
    assert cnt["reads"] == 3 and cnt["reads_multi"] == 1 and cnt["molecules"] == 1
    # selection by best de: b (0.05), a (0.1 -> its CCCC record); c dropped by MAXREADS; 2 reads, equal length -> s2
    assert fastq_records(fq) == [(b"@AAAA-M-3", b"CCCCCCCC", b"+", b"$" * 8)]


def test_last_record_gives_barcode_and_umi():
    recs = [rec("a", tags(umi="X", us="AAAAAA")), rec("a", tags(umi="Y", us="CCCCCC"), flag=2048), rec("b", tags(umi="X", us="GGGGGG"))]
    fq, cnt = run(recs)
    assert [r[0] for r in fastq_records(fq)] == [b"@AAAA-Y-1", b"@AAAA-X-1"]


def test_missing_sequence_stops_with_the_read_name():
    with pytest.raises(cm.ConsensusError, match="read lost"):
        run([rec("ok", tags(us="ACGTACGT")), rec("lost", tags())])
    run([rec("chim", tags(), cigar=[("S", 200), ("M", 4)])])              # a chimeric record is dropped before its sequence is read


def test_identical_reads_give_the_read_with_maxps():
    rng = np.random.default_rng(3)
    s = cm.random_seq(rng, 200)
    cons, qv = cm.molecule_consensus([s] * 5, 3, 20)
    assert cons == s and qv == bytes([53]) * 200


@pytest.mark.parametrize("kind", ["sub", "ins", "del"])
def test_minority_error_is_outvoted(kind):
    rng = np.random.default_rng(4)
    s = cm.random_seq(rng, 120)
    odd = {"sub": s[:60] + (b"A" if s[60:61] != b"A" else b"C") + s[61:], "ins": s[:60] + b"T" + s[60:], "del": s[:60] + s[61:]}[kind]
    for k in (3, 5, 8):
        for pos in range(k):
            reads = [s] * k
            reads[pos] = odd
            cons, qv = cm.molecule_consensus(reads, 3, 20)
            assert cons == s
            assert qv.count(bytes([53])) >= len(s) - 2


def test_every_read_path_spells_the_read():
    rng = np.random.default_rng(5)
    src = cm.random_seq(rng, 150)
    reads = [cm.noisy_copy(rng, src, 0.1) for _ in range(8)] + [b"", b"A", src[:20], cm.random_seq(rng, 40), b"NNNN"]
    g = cm.Graph()
    for r in reads:
        path = cm.add_read(g, r, cm.align(g, r))
        assert bytes(g.base[v] for v in path) == r
        for u, w in zip(path, path[1:]):
            assert any(g.e_to[e] == w for e in g.outs[u])
    assert sum(g.count) == sum(len(r) for r in reads)
    g.topo()                                                              # still a DAG


def test_empty_reads_add_nothing_but_count_as_rows():
    cons, qv = cm.molecule_consensus([b"ACGT", b"", b"ACGT"], 3, 20)
    assert cons == b"ACGT" and qv == bytes([cm.qv_byte(2, 3, 20)]) * 4
    assert cm.molecule_consensus([b"", b"", b""], 3, 20) == (b"", b"")


@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module("sicelore_amd.cli")


@pytest.mark.parametrize("argv,msg", [
    (["-I", "x.bam"], "missing required option"),
    (["O=out.fq"], "missing required option"),
    (["-I", "/nonexistent/x.bam", "-O", "o.fq"], "no such file"),
    (["I=/nonexistent/x.bam", "O=o.fq", "FOO=1"], "unknown option"),
    (["-I", "a", "-O", "b", "-MAPQV0", "yes"], "true or false"),
    (["-I", "a", "-O", "b", "-MAXREADS", "many"], "not a number"),
    (["-I", "a", "-O", "b", "-CELLTAG", "BCX"], "two-character"),
    (["-I", "a", "-O", "b", "-VALIDATION_STRINGENCY", "LAX"], "STRICT"),
    (["-I", "a", "-O"], "needs a value"),
    (["stray"], "unexpected argument"),
])
def test_cli_argument_errors(cli, capsys, argv, msg):
    assert cli.main(["ComputeConsensus"] + argv) == 1
    assert msg in capsys.readouterr().err


def test_cli_maxreads_below_one(cli, capsys, tmp_path):
    bam = tmp_path / "in.bam"
    bam.write_bytes(bammodel.bgzf_compress(bammodel.bam_bytes(HEAD, REFS, [])))
    assert cli.main(["ComputeConsensus", f"I={bam}", "O=" + str(tmp_path / "o.fq"), "MAXREADS=0"]) == 1
    assert "MAXREADS" in capsys.readouterr().err


def test_cli_other_programs_still_refused(cli, capsys):
    assert cli.main(["DeduplicateMolecule", "I=x"]) == 1
    err = capsys.readouterr().err
    assert "sub-command" in err and "DeduplicateMolecule" in err
