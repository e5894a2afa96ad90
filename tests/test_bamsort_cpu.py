"""BamSort without a GPU: the model of the order (tests/sortmodel.py) against a sorted stream written out by hand, the header rule, the
model's stop, the edges tests/test_bamsort_gpu.py claims asserted on its inputs (tests/sortcases.py), and bamsort.py's command line up
to the device call."""
import importlib
import struct

import pytest

import __graft_entry__ as graft
import bammodel
import sortcases as sc
import sortmodel as sm


def _mod(name):
    return importlib.import_module(f"{graft.PKG_NAME}.{name}")


@pytest.fixture(scope="module")
def lib(pkg):
    graft.build()
    return _mod("lib")


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, make in sc.CASES.items()}


def _segments(tmp_path, raw, segment_bytes):
    """the record counts of the segments the reader cuts `raw` into"""
    p = tmp_path / "seg.bam"
    p.write_bytes(raw)
    return [int(recs.size) for _bam, recs, _hdr in _mod("bamsegments").segments(str(p), segment_bytes, 1) if recs.size]


def _parsed(raw):
    return sm.split(bammodel.bgzf_decompress(raw))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_model_equals_the_stream_written_out_by_hand():
    refs = [("chrA", 1000), ("chrB", 1000)]
    R = dict(b5r=sc.rec("b5r", 1, 5, flag=16), u=sc.unplaced("u"), a9=sc.rec("a9", 0, 9), b5f=sc.rec("b5f", 1, 5), a9_too=sc.rec("a9_too", 0, 9),
             a_minus=sc.rec("a_minus", 0, -1))
    raw = bammodel.bgzf_compress(bammodel.bam_bytes("@HD\tVN:1.6\tSO:unsorted\n@CO\tx\n", refs, list(R.values())))
    text = b"@HD\tVN:1.6\tSO:coordinate\n@CO\tx\n"
    want = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", 2)
    want += struct.pack("<I", 5) + b"chrA\0" + struct.pack("<I", 1000) + struct.pack("<I", 5) + b"chrB\0" + struct.pack("<I", 1000)
    want += R["a_minus"] + R["a9"] + R["a9_too"] + R["b5f"] + R["b5r"] + R["u"]
    assert sm.sorted_stream(raw) == want


def test_header_rule():
    assert sm.header_text("@SQ\tSN:c\tLN:5\n") == "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c\tLN:5\n"
    assert sm.header_text("@HD\tVN:1.5\tSO:unsorted\n@SQ\tSN:c\tLN:5\n") == "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:c\tLN:5\n"
    assert sm.header_text("@HD\tVN:1.6\tSO:queryname\tGO:query\n") == "@HD\tVN:1.6\tSO:coordinate\tGO:query\n"
    assert sm.header_text("@HD\tVN:1.6\n@CO\tSO:unsorted\n") == "@HD\tVN:1.6\tSO:coordinate\n@CO\tSO:unsorted\n"
    assert sm.header_text("") == "@HD\tVN:1.6\tSO:coordinate\n"


def test_products_header_rule_is_the_models(pkg):
    """bamsort.sorted_header is host code: the same five texts, with l_text and the reference dictionary around them"""
    bs = _mod("bamsort")
    for text in ("@SQ\tSN:c\tLN:5\n", "@HD\tVN:1.5\tSO:unsorted\n@SQ\tSN:c\tLN:5\n", "@HD\tVN:1.6\tSO:queryname\tGO:query\n", "@HD\tVN:1.6\n@CO\tSO:unsorted\n", ""):
        hdr = bammodel.bam_bytes(text, [("c", 5)], [])
        assert bs.sorted_header(hdr) == bammodel.bam_bytes(sm.header_text(text), [("c", 5)], []), text


def test_stop_of_the_model():
    raw, _seg, _win, record, read = sc.stop()
    with pytest.raises(sm.SortStop) as e:
        sm.sorted_stream(raw)
    assert (e.value.record, e.value.read) == (record, read)


# ---- the edges the GPU test claims are in its inputs ---------------------------------------------------------------------------------------
def test_every_case_has_its_segments_and_windows(lib, cases, tmp_path):
    for name, (raw, seg, win) in cases.items():
        _hdr, recs = sm.sorted_records(bammodel.bgzf_decompress(raw))
        n = len(recs)
        assert sum(_segments(tmp_path, raw, 256 << 20)) == n, name
        assert len(_segments(tmp_path, raw, 256 << 20)) == min(n, 1), name
        many = _segments(tmp_path, raw, seg)
        assert sum(many) == n, name
        w = sm.windows([len(r) for r in recs], win)
        assert len(sm.windows([len(r) for r in recs], 64 << 20)) == min(n, 1), name
        if name in ("header_only", "one_record"):
            assert len(many) == n and len(w) == n, name
        else:
            assert len(many) >= 4 and len(w) >= 4 and win <= 4096, name


def test_hand_case_holds_its_edges(cases):
    raw = cases["hand"][0]
    _text, _dict, refs, recs = _parsed(raw)
    by = {r["name"]: r for r in recs}
    assert len(refs) == 3 and {r["ref_id"] for r in recs} >= {0, 1, 2, -1, -7}
    assert (by["none"]["ref_id"], by["none"]["pos0"]) == (-1, -1) and by["neg_ref"]["ref_id"] == -7
    assert (by["c1_minus1"]["ref_id"], by["c1_minus1"]["pos0"]) == (0, -1) and by["c1_max"]["pos0"] == 2 ** 31 - 1
    assert by["c1_flag4"]["flag"] & 4 and by["c1_flag4"]["ref_id"] == 0
    names = [r["name"] for r in recs]
    assert names.index("c2_rev_700") < names.index("c2_fwd_700") and names.index("c3_fwd_10") < names.index("c3_rev_10")
    for a, b in (("c2_rev_700", "c2_fwd_700"), ("c3_fwd_10", "c3_rev_10")):
        assert (by[a]["ref_id"], by[a]["pos0"]) == (by[b]["ref_id"], by[b]["pos0"]) and by[a]["flag"] ^ by[b]["flag"] == 16
    _hdr, out = sm.sorted_records(bammodel.bgzf_decompress(raw))
    assert [bammodel.parse_bam(_hdr + r)[2][0]["name"] for r in out] == sc.HAND_ORDER
    assert len(_parsed(cases["header_only"][0])[3]) == 0 and len(_parsed(cases["one_record"][0])[3]) == 1
    assert len(_parsed(cases["no_references"][0])[2]) == 0 and len(_parsed(cases["no_references"][0])[3]) == 60
    _t, _d, refs, recs = _parsed(cases["many_references"][0])
    assert len(refs) == 3000 and {0, 2999} <= {r["ref_id"] for r in recs} and any(r["ref_id"] < 0 for r in recs)


def test_tie_groups_and_the_group_across_a_border(lib, cases, tmp_path):
    raw, seg, _win = cases["ties"]
    _t, _d, refs, recs = _parsed(raw)
    groups = {}
    for i, r in enumerate(recs):
        groups.setdefault(sm.key(r, len(refs)), []).append(i)
    assert sorted(len(g) for g in groups.values()) == sorted(sc.TIE_GROUPS)
    assert len({r["name"] for r in recs}) == len(recs) == sum(sc.TIE_GROUPS)
    # the segment of every record in the segmented run: each larger group has records on both sides of a border
    counts = _segments(tmp_path, raw, seg)
    segment_of = [k for k, c in enumerate(counts) for _ in range(c)]
    for g in groups.values():
        if len(g) >= 63:
            assert len({segment_of[i] for i in g}) >= 2
    big = max(groups.values(), key=len)
    assert len({segment_of[i] for i in big}) == len(counts) >= 4
    # and the groups are interleaved in the input: the sort has to move them
    assert any(recs[i]["pos0"] > recs[i + 1]["pos0"] for i in range(len(recs) - 1))


def test_alignment_case_covers_all_256_pairs(cases):
    raw = cases["alignments"][0]
    _t, _d, refs, recs = _parsed(raw)
    first = recs[0]["off"]
    order = sorted(range(len(recs)), key=lambda i: sm.key(recs[i], len(refs)))
    pairs, at = set(), 0
    for i in order:
        pairs.add(((recs[i]["off"] - first) % 16, at % 16))
        at += recs[i]["length"]
    assert len(pairs) == 256
    assert {r["length"] for r in recs} == set(range(37, 85))


def test_length_case_holds_its_lengths_and_windows(cases):
    raw, _seg, win = cases["lengths"]
    _hdr, out = sm.sorted_records(bammodel.bgzf_decompress(raw))
    lens = [len(r) for r in out]
    assert set(sc.LENGTHS) <= set(lens)
    w = sm.windows(lens, win)
    assert w[0] == (0, 4, win)                                              # a window that ends exactly on its limit
    assert (lens.index(70000), lens.index(70000) + 1, 70000) in w and 70000 > win       # the long record: a window of its own
    assert [len(r) for r in _parsed(raw)[3]] != lens                        # the input has another order


def test_order_cases(cases):
    raw = cases["already_sorted"][0]
    assert sm.sorted_stream(raw) == bammodel.bgzf_decompress(raw)
    raw = cases["reversed_input"][0]
    _t, _d, refs, recs = _parsed(raw)
    keys = [sm.key(r, len(refs)) for r in recs]
    assert keys == sorted(keys, reverse=True) and len(set(keys)) == len(keys) > 1000


def test_seeded_case(lib, tmp_path):
    raw, refs = sc.seeded()
    _t, _d, _refs, recs = _parsed(raw)
    assert len(recs) == 20300 and sum(r["ref_id"] < 0 for r in recs) == 300 and {r["ref_id"] for r in recs} == {-1, 0, 1, 2, 3, 4}
    a, b = _segments(tmp_path, raw, 100_000), _segments(tmp_path, raw, 30_000)
    assert 4 <= len(a) < len(b)
    assert len(sm.windows([r["length"] for r in recs], 64 << 10)) >= 4


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def stubbed(pkg, monkeypatch):
    """bamsort.main with the device call replaced: the arguments it would run with"""
    bs, cli = _mod("bamsort"), _mod("cli")
    calls = []

    def fake(ctx, in_bam, out_bam, index=False, n_threads=4, **kw):
        calls.append((in_bam, out_bam, index, n_threads))
        return dict(records=6, segments=1, windows=1, bytes_written=300)
    monkeypatch.setattr(bs, "sort_bam", fake)
    monkeypatch.setattr(cli, "_context", lambda: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("SMI_ACTIVE_PROCESSORS", raising=False)
    return bs, calls


def test_command_line_argument_forms(stubbed, tmp_path, capsys):
    bs, calls = stubbed
    bam, out = tmp_path / "x.bam", str(tmp_path / "y.bam")
    bam.write_bytes(sc.one_record()[0])
    assert bs.main(["-o", out, str(bam)]) == 0
    assert bs.main(["-@", "3", "-o", out, str(bam)]) == 0
    assert bs.main(["-@8", str(bam), "-o", out, "--write-index"]) == 0
    assert bs.main(["-m", "768M", "-T", "/tmp/prefix", "-l", "5", "-@", "64", "-o", out, str(bam)]) == 0
    assert bs.main(["-m2G", "-l9", "-O", "bam", "-o", out, str(bam)]) == 0
    assert [c[:3] for c in calls] == [(str(bam), out, False), (str(bam), out, False), (str(bam), out, True), (str(bam), out, False), (str(bam), out, False)]
    assert [c[3] for c in calls[1:4]] == [3, 8, 16]
    assert "6 records in 1 segments, 1 windows, 300 bytes written" in capsys.readouterr().err
    assert bs.main([]) == 0
    text = capsys.readouterr().out
    assert "samtools sort" in text and "have no effect" in text


def test_command_line_refusals(stubbed, tmp_path, capsys, monkeypatch):
    bs, calls = stubbed
    bam, out = tmp_path / "x.bam", str(tmp_path / "y.bam")
    bam.write_bytes(sc.one_record()[0])
    for argv, text in ((["-n", "-o", out, str(bam)], "a sort by read name is not built"), (["-t", "CB", "-o", out, str(bam)], "a sort by tag is not built"),
                       (["-M", "-o", out, str(bam)], "the minimiser order is not built"), (["-O", "cram", "-o", out, str(bam)], "writes BAM alone"),
                       (["-O", "sam", "-o", out, str(bam)], "writes BAM alone"), ([str(bam)], "-o is missing"), (["-o", out, "-"], "not the standard input"),
                       (["-o", out, str(bam), str(bam)], "more than one input"), (["-o", out, str(tmp_path / "missing.bam")], "no such file"),
                       (["-o", str(tmp_path / "nodir" / "y.bam"), str(bam)], "no such directory"), (["-o", str(tmp_path), str(bam)], "a directory"),
                       (["-@", "x", "-o", out, str(bam)], "not a number"), (["-q", "-o", out, str(bam)], "unknown option"), (["-o", out], "usage"),
                       (["-o"], "needs a value")):
        assert bs.main(argv) == 1, argv
        assert text in capsys.readouterr().err, argv
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert bs.main(["-o", out, str(bam)]) == 1
    assert "start it without torchrun" in capsys.readouterr().err
    assert calls == []


def test_a_stop_is_exit_code_1_and_names_the_read(stubbed, tmp_path, capsys, monkeypatch):
    bs, _calls = stubbed
    lib = _mod("lib")

    def stop(*a, **k):
        raise lib.BamSortError("read beyond (record 25): its ref_id is not one of the header's references", "beyond", 25)
    monkeypatch.setattr(bs, "sort_bam", stop)
    bam, out = tmp_path / "x.bam", str(tmp_path / "y.bam")
    bam.write_bytes(sc.one_record()[0])
    assert bs.main(["-o", out, str(bam)]) == 1
    err = capsys.readouterr().err
    assert "read beyond (record 25)" in err and f"{out} was not written" in err


def test_cli_main_still_refuses_a_sort_sub_command(pkg, capsys):
    cli = _mod("cli")
    assert cli.main(["sort", "x.bam"]) == 1
    assert "this build has" in capsys.readouterr().err
