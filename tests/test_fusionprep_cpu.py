"""ExportClippedReads and AddBamReadTags without a GPU: tests/fusionprepmodel.py against a FASTQ and a tagged BAM written out by hand for
the hand-built cases of tests/fusionprepcases.py, the records the reference's loop dies on, the command line of fusionprep.py up to the
point where it asks for a device, and that every edge tests/test_fusionprep_gpu.py claims is in its input."""
import importlib
import inspect
import os

import pytest

import bammodel
import fusionprepcases as pc
import fusionprepmodel as m
import tagbammodel as tm


@pytest.fixture(scope="module")
def fp(pkg):
    return importlib.import_module("sicelore_amd.fusionprep")


@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module("sicelore_amd.cli")


def _fq(key, us="ACGT", qs="IIII"):
    return f"@{key}\n{us}\n+\n{qs}\n".encode()


# the FASTQ of pc.hand_records(), record by record in file order
HAND_FASTQ = b"".join([
    _fq("s151_G_C_U", "AAAA", "!!!!"), _fq("e151_G_C_U"), _fq("h151_G_C_U"), _fq("g151_G_C_U"),      # 151 at each end; 150 is not clipped
    _fq("one_G_C_U"),                                                                              # 200S alone; 5H200S100M is not clipped
    _fq("noge_null_C_U"), _fq("nobc_G_null_U"), _fq("noumi_G_C_null"),
    _fq("nous_G_C_U", "null"), _fq("noqs_G_C_U", qs="null"), _fq("uneq_G_C_U", "ACGTACGT", "II"), _fq("empty_G_C_U", "", "III"),
    _fq("_G_C_U"), _fq("_GE2_C_U"),                                                                # "_lead_x" and the empty name
    _fq("dup_GD_C_U", "AC", "II"),                                                                 # dup_b and dup_c lose
    _fq("nc_GN_C_U", "TTTT", "KKKK"),                                                              # nc_1 reserved nothing
    _fq("fu_GF_C_U", "null"),                                                                      # fu_2 (with US) loses
    _fq("eq_G_C_U"), _fq("eq2_G_C_U"),
    _fq("rep_G_last_U"), _fq("a_b_c_x_U"),                                                         # a_z has the same key out of other fields
])


def test_model_writes_the_hand_written_fastq():
    fastq, counts, decisions = m.export_clipped_reads(pc.hand_bam())
    assert fastq == HAND_FASTQ
    assert counts == dict(records=32, clipped=25, written=21)
    names = [r["name"] for r in bammodel.parse_bam(pc.hand_bam())[2]]
    dec = dict(zip(names, decisions))
    assert dec["s150_x"] == dec["e150"] == dec["h150"] == dec["g150"] == dec["inner"] == dec["one150"] == dec["nc_1"] == (False, False)
    assert dec["dup_b"] == dec["dup_c"] == dec["fu_2"] == dec["a_z"] == (True, False)
    assert dec["one"] == dec["eq"] == dec[""] == dec["_lead_x"] == (True, True)


def test_minclip_is_strict_and_a_java_int():
    bam = pc.hand_bam()
    assert m.export_clipped_reads(bam, min_clip=149)[1]["clipped"] == 25 + 5           # s150_x e150 h150 g150 one150
    assert m.export_clipped_reads(bam, min_clip=200)[1] == dict(records=32, clipped=1, written=1)     # nc_2's 300S
    assert m.export_clipped_reads(bam, min_clip=-1)[1]["clipped"] == 32 - 1            # all but nc_1 (10M): the 5H of inner counts now
    assert m.export_clipped_reads(pc.bam([pc.rec("z", [("S", 0), ("M", 5)])]), min_clip=-1)[1]["clipped"] == 1


def test_option_tags_are_read():
    recs = [pc.rec("r_1", pc.S200, extra=tm.aux_z("XG", "g2") + tm.aux_z("XC", "c2") + tm.aux_z("XU", "u2") + tm.aux_z("XS", "TT") + tm.aux_z("XQ", "##"))]
    assert m.export_clipped_reads(pc.bam(recs), gene_tag="XG", cell_tag="XC", umi_tag="XU", us_tag="XS", qs_tag="XQ")[0] == b"@r_g2_c2_u2\nTT\n+\n##\n"
    assert m.export_clipped_reads(pc.bam(recs), gene_tag="BC", cell_tag="BC", umi_tag="BC", us_tag="QS", qs_tag="QS")[0] == b"@r_C_C_C\nIIII\n+\nIIII\n"


@pytest.mark.parametrize("which,read", [("underscores", "___"), ("a_typed_bc", "abc"), ("h_typed_us", "hus"), ("int_typed_qs", "iqs"),
                                        ("no_cigar", "nocigar"), ("eq_clip", "eqclip"), ("eq_clip_2", "eqclip2")])
def test_stop_cases_name_their_read(which, read):
    with pytest.raises(m.Stop) as e:
        m.export_clipped_reads(pc.stop_bam(which))
    assert (e.value.read, e.value.record) == (read, 20)


def test_what_does_not_stop():
    """an A-typed BC stops on a record that is not clipped (above); a US / QS that is no string stops only where it would be written"""
    R = pc.hand_records()
    hus = pc.STOPS["h_typed_us"]()
    fastq, counts, _ = m.export_clipped_reads(pc.bam(R + [pc.rec("hus_first", pc.S200, ge="GH"), hus]))     # its key was written already
    assert fastq == HAND_FASTQ + _fq("hus_GH_C_U") and counts["clipped"] == 27
    notclipped = pc.rec("hus", pc.M10, ge="GH", us=None, extra=tm.aux_h("US", "abcd"))
    assert m.export_clipped_reads(pc.bam(R + [notclipped]))[0] == HAND_FASTQ
    with pytest.raises(m.Stop):
        m.export_clipped_reads(pc.bam(R + [hus]))
    # a leading clip in front of '=' and a trailing clip behind "=, M" are in the hand-built case; '=' alone and '=' first are fine too
    ok = [pc.rec("e1", [("=", 30)]), pc.rec("e2", [("=", 30), ("S", 200), ("M", 1)]), pc.rec("e3", [("S", 200), ("=", 30), ("M", 1)])]
    assert m.export_clipped_reads(pc.bam(ok))[1] == dict(records=3, clipped=1, written=1)


# ---- AddBamReadTags ---------------------------------------------------------------------------------------------------------------------
def test_split_of_the_read_name():
    want = {"a_b": None, "g_c_u": ("g", "c", "u"), "x_g_c_u": ("g", "c", "u"), "a_b_c_d_e": None, "a_b_c_": ("a", "b", "c"), "a_b__": None,
            "_a_b": ("", "a", "b"), "a__b_c": ("", "b", "c"), "___": None, "": None, "GENE1_CELLACGT_UMI12345": ("GENE1", "CELLACGT", "UMI12345"),
            "r1_GENE1_CELL_UMI": ("GENE1", "CELL", "UMI"), "null_null_null": ("null", "null", "null")}
    assert sorted(want) == sorted(pc.READ_NAMES)
    for name, w in want.items():
        assert m.read_edits(name) == ([] if w is None else list(zip(("GE", "BC", "U8"), w))), name
    assert m.read_edits("MY_GENE_c_u") == [("GE", "GENE"), ("BC", "c"), ("U8", "u")]          # a gene name with '_' shifts the pieces, as in the reference
    assert m.read_edits("A_MY_GENE_c_u") == []


def _z(tag, v):
    return tm.aux_z(tag, v)


def test_model_writes_the_hand_written_bam():
    """attributes in htsjdk's order (by the tag's second character, then its first): U8 < AA < BC < GE < NM < ZZ"""
    nm2 = tm.aux_int("NM", "c", 2)                                                          # written in the smallest type, signed first
    want_aux = [
        b"",                                                                               # a_b
        _z("U8", "u") + _z("BC", "c") + _z("GE", "g") + nm2,                               # g_c_u over GE:Z:old BC:C:5 U8:Z:old NM
        _z("U8", "u") + _z("AA", "x") + _z("BC", "c") + _z("GE", "g") + _z("ZZ", "y"),     # x_g_c_u beside AA and ZZ
        b"",                                                                               # a_b_c_d_e (unmapped)
        _z("U8", "c") + _z("BC", "b") + _z("GE", "a") + nm2,                               # a_b_c_
        _z("AA", "x") + _z("ZZ", "y"),                                                     # a_b__
        _z("U8", "b") + _z("BC", "a") + _z("GE", ""),                                      # _a_b: an empty piece is an empty string
        _z("U8", "c") + _z("BC", "b") + _z("GE", "") + nm2,                                # a__b_c (unmapped)
        _z("AA", "x") + _z("ZZ", "y"),                                                     # ___
        b"",                                                                               # the empty name
        _z("U8", "UMI12345") + _z("BC", "CELLACGT") + _z("GE", "GENE1") + nm2,
        _z("U8", "UMI") + _z("AA", "x") + _z("BC", "CELL") + _z("GE", "GENE1") + _z("ZZ", "y"),   # (unmapped)
        _z("U8", "null") + _z("BC", "null") + _z("GE", "null"),
    ]
    want = pc.bam([bammodel.bam_record(nm, 4 if k % 4 == 3 else 0, -1 if k % 4 == 3 else 0, 100 + k, 60, [] if k % 4 == 3 else pc.M10, "ACGT", aux=want_aux[k])
                   for k, nm in enumerate(pc.READ_NAMES)])
    got, cnt = m.add_bam_read_tags(pc.read_bam())
    assert got == want and cnt == dict(records=13, tagged=8)


def test_coinciding_tag_options_keep_the_later_one():
    one = pc.bam([bammodel.bam_record("g_c_u", 0, 0, 1, 60, pc.M10, "ACGT")])
    for opt, aux in ((dict(gene="XX", cell="XX", umi="YY"), _z("XX", "c") + _z("YY", "u")), (dict(gene="XX", cell="YY", umi="XX"), _z("XX", "u") + _z("YY", "c")),
                     (dict(gene="XX", cell="XX", umi="XX"), _z("XX", "u"))):
        assert m.add_bam_read_tags(one, **opt)[0] == pc.bam([bammodel.bam_record("g_c_u", 0, 0, 1, 60, pc.M10, "ACGT", aux=aux)])


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_cli_main_still_refuses_both_names(cli, capsys):
    for sub in ("ExportClippedReads", "AddBamReadTags"):
        assert cli.main([sub, "I=x.bam", "O=y"]) == 1
        assert "this build has" in capsys.readouterr().err


def test_both_syntaxes_and_the_defaults(fp, cli, monkeypatch, tmp_path):
    (tmp_path / "in.bam").write_bytes(b"")
    calls = []
    monkeypatch.setattr(cli, "_context", lambda: "ctx")
    monkeypatch.setattr(fp, "export_clipped_reads", lambda ctx, i, o, **kw: calls.append(("E", i, o, kw)) or dict(records=0, clipped=0, written=0))
    monkeypatch.setattr(fp, "add_bam_read_tags", lambda ctx, i, o, **kw: calls.append(("A", i, o, kw)) or dict(records=0, tagged=0))
    src, fq, dst = str(tmp_path / "in.bam"), str(tmp_path / "o.fastq"), str(tmp_path / "o.bam")
    assert fp.main(["ExportClippedReads", f"I={src}", f"O={fq}"]) == 0
    assert fp.main(["ExportClippedReads", "-I", src, "--OUTPUT", fq, "-MINCLIP", "7", "-CELLTAG=XC", "UMITAG=XU", "GENETAG=XG", "USTAG=XS", "QSTAG=XQ",
                    "VALIDATION_STRINGENCY=SILENT"]) == 0
    assert fp.main(["AddBamReadTags", f"INPUT={src}", f"O={dst}"]) == 0
    assert fp.main(["AddBamReadTags", "-I", src, "-O", dst, "-GENETAG", "XG", "CELLTAG=XC", "--UMITAG", "XU", "-VALIDATION_STRINGENCY", "LENIENT"]) == 0
    for c in calls:
        c[3].pop("n_threads")
    defaults = dict(min_clip=150, cell_tag="BC", umi_tag="U8", gene_tag="GE", us_tag="US", qs_tag="QS")
    assert calls == [("E", src, fq, defaults), ("E", src, fq, dict(min_clip=7, cell_tag="XC", umi_tag="XU", gene_tag="XG", us_tag="XS", qs_tag="XQ")),
                     ("A", src, dst, dict(gene_tag="GE", cell_tag="BC", umi_tag="U8")), ("A", src, dst, dict(gene_tag="XG", cell_tag="XC", umi_tag="XU"))]
    # the same defaults in the functions' signatures and in the library's config
    monkeypatch.undo()
    sig = inspect.signature(fp.export_clipped_reads).parameters
    assert {k: sig[k].default for k in defaults} == defaults and sig["table_log2"].default == 0 and sig["segment_bytes"].default == 256 << 20
    sig = inspect.signature(fp.add_bam_read_tags).parameters
    assert {k: sig[k].default for k in ("gene_tag", "cell_tag", "umi_tag")} == dict(gene_tag="GE", cell_tag="BC", umi_tag="U8")
    lib = importlib.import_module("sicelore_amd.lib")
    cfg = lib.ClipExport.__new__(lib.ClipExport)._config({})
    assert (cfg.min_clip, cfg.cell_tag, cfg.umi_tag, cfg.gene_tag, cfg.us_tag, cfg.qs_tag, cfg.table_log2, cfg.keep_records) == (150, b"BC", b"U8", b"GE", b"US", b"QS", 0, 0)
    cfg = lib.MolTag.__new__(lib.MolTag)._config({}, lib.MOLTAG_READ)
    assert (cfg.program, cfg.gene_tag, cfg.cell_tag, cfg.umi_tag) == (2, b"GE", b"BC", b"U8")


def test_argument_errors_exit_1(fp, capsys, monkeypatch, tmp_path):
    (tmp_path / "in.bam").write_bytes(b"")
    src = str(tmp_path / "in.bam")

    def err(argv):
        assert fp.main(argv) == 1
        return capsys.readouterr().err

    assert "missing required option(s) I, O" in err(["ExportClippedReads"])
    assert "missing required option(s) O" in err(["ExportClippedReads", f"I={src}"])               # optional in the reference, which then opens it
    assert "missing required option(s) I" in err(["AddBamReadTags", "O=x.bam"])
    assert "missing required option(s) O" in err(["AddBamReadTags", f"I={src}"])
    for prog, tags in (("ExportClippedReads", ("CELLTAG", "UMITAG", "GENETAG", "USTAG", "QSTAG")), ("AddBamReadTags", ("CELLTAG", "UMITAG", "GENETAG"))):
        for tag in tags:
            for bad in ("B", "BCX", ""):
                assert "is not a two-character tag" in err([prog, f"I={src}", "O=" + str(tmp_path / "o.bam"), f"{tag}={bad}"])
    assert "MINCLIP 'x' is not a number" in err(["ExportClippedReads", f"I={src}", "O=o.fq", "MINCLIP=x"])
    assert "is not a number" in err(["ExportClippedReads", f"I={src}", "O=" + str(tmp_path / "o.fq"), "MINCLIP=2147483648"])
    assert "unknown option 'FASTQ'" in err(["ExportClippedReads", f"I={src}", "O=o.fq", "FASTQ=x"])
    assert "no such file" in err(["ExportClippedReads", "I=" + str(tmp_path / "none.bam"), "O=" + str(tmp_path / "o.fq")])
    assert "no such file" in err(["AddBamReadTags", "I=" + str(tmp_path / "none.bam"), "O=" + str(tmp_path / "o.bam")])
    assert "no such directory" in err(["ExportClippedReads", f"I={src}", "O=" + str(tmp_path / "nodir" / "o.fq")])
    assert "fusionprep.py has ExportClippedReads and AddBamReadTags" in err(["AddBamReadSequenceTag", f"I={src}"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "ExportClippedReads runs in one process on one GPU" in err(["ExportClippedReads", f"I={src}", "O=" + str(tmp_path / "o.fq")])
    assert "AddBamReadTags runs in one process on one GPU" in err(["AddBamReadTags", f"I={src}", "O=" + str(tmp_path / "o.bam")])
    assert os.listdir(tmp_path) == ["in.bam"]


# ---- the inputs of the GPU tests hold the edges they claim ------------------------------------------------------------------------------
def _offsets(fastq):
    """per record of a FASTQ whose sequences hold no newline: (offset of '@', of the sequence, of the qualities, lengths of key, US, QS)"""
    out, p = [], 0
    while p < len(fastq):
        e1 = fastq.index(b"\n", p)
        e2 = fastq.index(b"\n", e1 + 1)
        e4 = fastq.index(b"\n", e2 + 3)
        out.append((p, e1 + 1, e2 + 3, e1 - p - 1, e2 - e1 - 1, e4 - e2 - 3))
        p = e4 + 1
    return out


def test_lengths_case_reaches_every_length_at_every_alignment():
    fastq, counts, _ = m.export_clipped_reads(pc.lengths_case())
    assert counts == dict(records=48, clipped=48, written=48)
    seen_us, seen_qs, seen_key = set(), set(), set()
    for at, seq, qual, klen, us, qs in _offsets(fastq):
        seen_us.add((us, seq % 4))
        seen_qs.add((qs, qual % 4))
        seen_key.add((at + 1) % 4)
    assert seen_us == {(L, a) for L in pc.LENGTHS for a in range(4)}
    assert {L for L, _a in seen_qs} == set(pc.LENGTHS) and {a for _L, a in seen_qs} == {0, 1, 2, 3} == seen_key
    assert max(pc.LENGTHS) > 0xFF00                                              # a record larger than a BGZF block


def test_key_and_table_cases_hold_their_edges():
    fastq, counts, dec = m.export_clipped_reads(pc.dup_case())
    assert counts == dict(records=sum(pc.DUP_SIZES), clipped=sum(pc.DUP_SIZES), written=len(pc.DUP_SIZES))
    assert [ln for ln in fastq.split(b"\n")[1::4]] == [b"ACGTN0"] * 5            # the first record of each key
    names = [r["name"] for r in bammodel.parse_bam(pc.dup_case())[2]]
    assert names.index("d65_64") == len(names) - 1 and names.index("d65_1") < 10     # the groups are spread over the file
    fastq, counts, _ = m.export_clipped_reads(pc.prefix_case())
    keys = [ln[1:] for ln in fastq.split(b"\n")[0::4] if ln]
    assert counts["written"] == len(set(keys)) == len(keys) == 16 + 2 and counts["clipped"] == 40     # p___ and, three times, p____
    assert {b"ab_G_C_AAAA", b"abc_G_C_AAAA", b"ab_G_C_AAAB", b"ab_G_C_AAA", b"p___", b"p____"} <= set(keys)
    for n, wrap, dups in ((64, 0, False), (200, 3, True)):
        fastq, counts, _ = m.export_clipped_reads(pc.distinct_case(n, wrap, dups))
        assert counts["written"] == n and counts["clipped"] == (2 * n - wrap if dups else n)
    for u in pc.last_slot_umis(3):
        key = f"w_G_C_{u}".encode()
        assert all(pc.slot(key, s) == s - 1 for s in (16, 128, 256, 512))         # the last slot of every table the case goes through
    assert pc.fnv1a(b"") == 0xcbf29ce484222325 and pc.fnv1a(b"a") == 0xaf63dc4c8601ec8c      # FNV-1a's published test vectors
    assert m.export_clipped_reads(pc.none_clipped_case())[:2] == (b"", dict(records=100, clipped=0, written=0))
    assert m.export_clipped_reads(pc.bam([]))[:2] == (b"", dict(records=0, clipped=0, written=0))


def test_seeded_case_is_mixed():
    bam = pc.seeded_case(5)
    fastq, counts, _ = m.export_clipped_reads(bam)
    assert counts["records"] == 20000 and 5000 < counts["clipped"] < 8000 and 2000 < counts["written"] < counts["clipped"] - 1000
    assert fastq.count(b"_null_") > 50 and fastq.count(b"\nnull\n") > 50
    assert pc.seeded_case(5) == bam


def test_chain_case_makes_fusions():
    import fusionmodel as fm

    fastq, counts, _ = m.export_clipped_reads(pc.bam(pc.chain_records()))
    assert counts == dict(records=60, clipped=48, written=48)
    tagged, cnt = m.add_bam_read_tags(pc.remapped_bam(fastq))
    assert cnt == dict(records=48, tagged=48)
    files, fc, fusions, _mols = fm.fusion_detector(tagged, pc.CHAIN_CSV)
    assert fc["valid"] == 48 and dict(fusions) == {"BCR|ABL1": fc["counted"]} and fc["counted"] >= 10
