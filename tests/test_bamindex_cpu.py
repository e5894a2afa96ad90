"""BamIndex without a GPU: the model of the index (tests/baimodel.py) against a .bai written out by hand and against bammodel.bai_bytes
where both can say the same, the consumer of the index (assignumis.bai_ref_extents_bytes) on the model's bytes, the cover property of the
specification's reader on every case and on 200 seeded regions, the edges tests/test_bamindex_gpu.py claims asserted on its inputs, the
host function smi_bgzf_block_table, the reader's block tables, and bamindex.py's command line up to the device call."""
import importlib
import struct

import numpy as np
import pytest

import __graft_entry__ as graft
import baicases as bc
import baimodel as bm
import bammodel


def _mod(name):
    return importlib.import_module(f"{graft.PKG_NAME}.{name}")


@pytest.fixture(scope="module")
def lib(pkg):
    graft.build()
    return _mod("lib")


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, make in bc.CASES.items()}


@pytest.fixture(scope="module")
def seeded():
    raw = bc.seeded()
    return raw, bm.bai_model(raw)


def _segments(tmp_path, raw, segment_bytes):
    """the record counts of the segments the reader cuts `raw` into"""
    p = tmp_path / "seg.bam"
    p.write_bytes(raw)
    return [int(recs.size) for _bam, recs, _hdr in _mod("bamsegments").segments(str(p), segment_bytes, 1) if recs.size]


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_model_equals_the_index_written_out_by_hand():
    raw, _seg = bc.hand()
    b0 = struct.unpack_from("<H", raw, 16)[0] + 1                  # BSIZE of the first block: where the second one starts
    blocks = bm.bgzf_walk(raw)
    assert [(c, len(p)) for c, _s, p in blocks][:2] == [(0, 100), (b0, 60)] and [len(p) for _c, _s, p in blocks] == [100, 60, 38, 0]
    # header [0, 50), a [50, 107), b [107, 157), c [157, 198): a starts in block 0 and ends 7 bytes into block 1
    second = b0 << 16
    want = b"BAI\x01" + struct.pack("<i", 1)
    want += struct.pack("<i", 3)
    want += struct.pack("<Ii", 4681, 1) + struct.pack("<QQ", 50, second | 7)                  # a: [100, 110), window 0
    want += struct.pack("<Ii", 4682, 1) + struct.pack("<QQ", second | 7, second | 57)         # b: [20000, 20005), window 1
    want += struct.pack("<Ii", 37450, 2) + struct.pack("<QQ", 50, second | 57) + struct.pack("<QQ", 2, 0)
    want += struct.pack("<i", 2) + struct.pack("<QQ", 50, second | 7)
    want += struct.pack("<Q", 1)                                                              # c has no reference
    assert bm.bai_model(raw) == want
    assert len(want) == 8 + 4 + 3 * 8 + 4 * 16 + 4 + 16 + 8


def test_model_equals_bammodels_index_where_both_can_say_it(cases, seeded):
    """bammodel.bai_bytes counts every placed record as mapped and writes no n_no_coor: inputs without a placed flag 0x4, trailer stripped"""
    for name in ("hand", "offsets", "chunks", "linear", "many_references", "only_unplaced"):
        raw = cases[name][0]
        refs, recs = bm.records_of(raw)
        assert not any(r[0] >= 0 and r[3] & 4 for r in recs), name
        idx = [(r[0], r[1], r[2], r[4], r[5]) for r in recs]
        assert bm.bai_model(raw)[:-8] == bammodel.bai_bytes(len(refs), idx, meta=True), name


def test_the_consumer_reads_the_models_extents(pkg, cases, seeded):
    au = _mod("assignumis")
    for name, raw in [(k, v[0]) for k, v in cases.items()] + [("seeded", seeded[0])]:
        refs, recs = bm.records_of(raw)
        want = []
        for r in range(len(refs)):
            mine = [x for x in recs if x[0] == r]
            want.append((min(x[4] for x in mine), max(x[5] for x in mine)) if mine else None)
        assert au.bai_ref_extents_bytes(bm.bai_model(raw)) == want, name


def test_reader_finds_every_overlapping_record(cases, seeded):
    for name, (raw, _seg) in cases.items():
        refs, _recs = bm.records_of(raw)
        regions = bc.random_regions(refs, 200, seed=len(name)) if refs else []
        assert bm.uncovered(raw, bm.bai_model(raw), regions) == [], name
    raw, bai = seeded
    assert bm.uncovered(raw, bai, bc.random_regions(bm.records_of(raw)[0], 200)) == []


def test_reader_misses_a_record_when_a_chunk_is_cut():
    """the cover check can fail: the same index with the first chunk ending one byte early"""
    raw, _seg = bc.hand()
    bai = bytearray(bm.bai_model(raw))
    at = 8 + 4 + 8 + 8                                  # the end of bin 4681's chunk
    struct.pack_into("<Q", bai, at, struct.unpack_from("<Q", bai, at)[0] - 1)
    assert bm.uncovered(raw, bytes(bai)) == [((0, 100, 110), 0)]


def test_stops_of_the_model():
    for name, (raw, _seg, record, read, kind) in bc.stops().items():
        with pytest.raises(bm.BaiStop) as e:
            bm.bai_model(raw)
        assert (e.value.record, e.value.read, e.value.kind) == (record, read, kind), name


# ---- the edges the GPU test claims are in its inputs ---------------------------------------------------------------------------------------
def _level(b):
    return sum(b >= base for base in (1, 9, 73, 585, 4681))


def test_extents_case_holds_its_edges(cases):
    raw, _seg = cases["extents"]
    refs, recs = bm.records_of(raw)
    by = {r[6]: r for r in recs}
    data, _voff = bm.offsets_of(raw)
    n_cigar = {r["name"]: len(r["cigar"]) for r in bammodel.parse_bam(data)[2]}
    assert [n_cigar[f"ops{n}"] for n in (0, 1, 63, 64, 65, 300, 65535)] == [0, 1, 63, 64, 65, 300, 65535]
    assert by["ops0"][2] - by["ops0"][1] == 1 and by["onlySI"][2] - by["onlySI"][1] == 1 and by["placed4"][2] - by["placed4"][1] == 1
    assert by["placed4"][3] & 4 and by["cgplaceholder"][2] - by["cgplaceholder"][1] == 5000
    for k, lvl in ((14, 5), (17, 4), (20, 3), (23, 2), (26, 1)):
        on, across = by[f"ends_on_2^{k}"], by[f"across_2^{k}"]
        assert on[2] == 1 << k and across[1] < 1 << k <= across[2] - 1
        assert _level(bammodel.reg2bin(on[1], on[2])) == 5 and _level(bammodel.reg2bin(across[1], across[2])) == lvl - 1
    assert by["end_2^29"][2] == 1 << 29 and by["pos_2^29-1"][1] == (1 << 29) - 1 and by["pos_2^29-1"][2] == 1 << 29
    sk = by["skip_2^27"]
    assert ((sk[2] - 1) >> 14) - (sk[1] >> 14) + 1 == 8193
    levels = {_level(bammodel.reg2bin(r[1], r[2])) for r in recs}
    assert levels == {0, 1, 2, 3, 4, 5}
    parsed, no_coor = bm.parse_bai(bm.bai_model(raw))
    assert no_coor == 0 and len(parsed[0]["lin"]) == 1 << 15 and parsed[0]["meta"][1] == (len(recs) - 1, 1)


def test_offsets_case_holds_its_edges(cases):
    for name in ("offsets", "offsets_border"):
        raw, _seg = cases[name]
        blocks = bm.bgzf_walk(raw)
        assert blocks[-1][2] != b""                                           # no EOF block
        empty = [k for k, b in enumerate(blocks) if not b[2]]
        assert len(empty) == 1 and 0 < empty[0] < len(blocks) - 1             # one empty block, in mid-file
        _refs, recs = bm.records_of(raw)
        by = {r[6]: r for r in recs}
        starts = {b[0] << 16 for b in blocks if b[2]}
        assert by["fills"][4] in starts and by["fills"][5] in starts          # first byte of a block to the last byte of it
        assert by["fills"][5] == by["spans3"][4]
        sp = by["spans3"]
        assert len({b[0] for b in blocks if sp[4] >> 16 <= b[0] <= sp[5] >> 16 and b[2]}) == 3
        be = by["before_empty"]
        assert be[5] & 0xffff == 0 and be[5] >> 16 == blocks[empty[0] + 1][0]  # behind it: the block behind the empty one
        assert recs[-1][5] == len(raw) << 16                                  # behind the last byte: the end of the file


def test_offsets_border_case_cuts_where_it_says(pkg, cases, tmp_path):
    raw, seg = cases["offsets_border"]
    blocks = bm.bgzf_walk(raw)
    empty = next(k for k, b in enumerate(blocks) if not b[2])
    assert blocks[empty][0] == seg                                            # the first read ends in front of the empty block
    counts = _segments(tmp_path, raw, seg)
    assert counts[0] == 3 and len(counts) >= 4                                # ... behind "before_empty"


def test_chunks_case_holds_its_edges(pkg, cases, tmp_path):
    raw, seg = cases["chunks"]
    _refs, recs = bm.records_of(raw)
    runs, last = [], None
    for r in recs:
        key = (r[0], bammodel.reg2bin(r[1], r[2]))
        if key == last:
            runs[-1][1] += 1
        else:
            runs.append([key[1], 1])
        last = key
    lengths = [n for _b, n in runs]
    assert lengths[:6] == [1, 1, 2, 63, 64, 65] and lengths[6:136] == [1] * 130 and lengths[136:] == [3000, 1]
    assert [b for b, _n in runs[6:136]] == [4691, 586] * 65
    assert runs[0][0] == 0 and runs[-1][0] == 0                               # bin 0: a chunk from the first and one from the last segment
    counts = _segments(tmp_path, raw, seg)
    assert len(counts) >= 4
    first_long = sum(lengths[:136])
    borders = np.cumsum(counts)[:-1]
    assert int(((borders > first_long) & (borders < first_long + 3000)).sum()) >= 2      # the long run crosses two segment borders
    parsed, _n = bm.parse_bai(bm.bai_model(raw))
    assert len(parsed[0]["bins"][0]) == 2 and len(parsed[0]["bins"][4691]) == 65 and len(parsed[0]["bins"][4701]) == 1


def test_reference_and_linear_cases_hold_their_edges(cases):
    parsed, no_coor = bm.parse_bai(bm.bai_model(cases["no_references"][0]))
    assert parsed == [] and no_coor == 0
    parsed, no_coor = bm.parse_bai(bm.bai_model(cases["only_unplaced"][0]))
    assert [(p["bins"], p["meta"], p["lin"]) for p in parsed] == [({}, None, [])] * 2 and no_coor == 40
    parsed, no_coor = bm.parse_bai(bm.bai_model(cases["many_references"][0]))
    assert len(parsed) == 3000 and [r for r, p in enumerate(parsed) if p["meta"]] == list(range(1, 3000, 3))
    assert parsed[0]["meta"] is None and parsed[2999]["meta"] is None and all(len(p["lin"]) == 2 for p in parsed[1::3])
    parsed, _n = bm.parse_bai(bm.bai_model(cases["linear"][0]))
    lin = parsed[0]["lin"]
    assert lin[:5] == [0] * 5 and lin[5] != 0                                  # leading empty windows
    assert lin[6:16] == [lin[5]] * 10 and lin[16] > lin[5]                     # a gap of 10 windows takes the value in front
    w = 100 + 8193 - 1
    assert len(set(lin[100:w + 1])) == 1 and lin[99] < lin[100] < lin[w + 1] if len(lin) > w + 1 else True
    assert len(lin) == ((100 << 14) + 16000 + 10 + (1 << 27) - 1 >> 14) + 1


def test_every_case_is_read_in_four_segments_or_more(pkg, cases, tmp_path):
    for name, (raw, seg) in cases.items():
        if name in ("no_references", "hand"):
            continue                                                          # (no record; three records)
        assert len(_segments(tmp_path, raw, seg)) >= 4, name
    assert _segments(tmp_path, cases["hand"][0], cases["hand"][1]) == [2, 1]
    for name, (raw, seg, record, _read, _kind) in bc.stops().items():
        counts = _segments(tmp_path, raw, seg)
        assert len(counts) >= 4, name
        if name == "pos_decreases_at_border":
            assert counts[0] == record                                        # the record that steps back is the second segment's first
        if name == "pos_decreases_inside":
            assert record not in np.cumsum(counts)


# ---- the host layer ------------------------------------------------------------------------------------------------------------------------
def test_block_table_reads_bsize_and_isize(lib, cases):
    for name in ("offsets", "extents", "hand"):
        raw = cases[name][0]
        data = np.frombuffer(raw, dtype=np.uint8)
        coff, isize, used = lib.bgzf_block_table(data, base=1000)
        want = bm.bgzf_walk(raw)
        assert used == len(raw) and coff.tolist() == [1000 + c for c, _s, _p in want] and isize.tolist() == [len(p) for _c, _s, p in want], name
        cut = data[:len(raw) - 5]                                             # an incomplete last block is left to the caller
        coff, isize, used = lib.bgzf_block_table(cut)
        assert len(coff) == len(want) - 1 and used == want[-1][0]
    damaged = bytearray(raw)
    damaged[0] = 0
    with pytest.raises(lib.SmiError, match="not a BGZF block"):
        lib.bgzf_block_table(np.frombuffer(bytes(damaged), dtype=np.uint8))
    coff, isize, used = lib.bgzf_block_table(np.zeros(0, dtype=np.uint8))
    assert coff.size == 0 and isize.size == 0 and used == 0


def test_reader_hands_out_block_tables_and_stream_offsets(pkg, cases, tmp_path):
    """the blocks keyword: all tables together are the file's, each segment's bytes start at the stream offset it comes with, and the
    yielded triples are those of a call without the keyword"""
    seg_mod = _mod("bamsegments")
    for name in ("offsets", "chunks", "hand"):
        raw, seg = cases[name]
        p = tmp_path / f"{name}.bam"
        p.write_bytes(raw)
        stream = b"".join(b[2] for b in bm.bgzf_walk(raw))
        got, offs = [], []

        carried = []

        def on_blocks(coff, isize, end, stream_off):
            carried.append(sum(n for _c, n in got) - stream_off)              # bytes of a record cut by the border in front
            got.extend(zip(coff.tolist(), isize.tolist()))
            offs.append((stream_off, end))
        n = 0
        plain = list(seg_mod.segments(str(p), seg, 1))
        for k, (bam, recs, hdr) in enumerate(seg_mod.segments(str(p), seg, 1, blocks=on_blocks)):
            assert bam.tobytes() == stream[offs[-1][0]:offs[-1][0] + bam.size], name
            assert bam.tobytes() == plain[k][0].tobytes() and recs.tobytes() == plain[k][1].tobytes() and hdr == plain[k][2]
            n += 1
        assert n == len(plain) and offs[-1][1] == len(raw)
        assert min(carried) >= 0 and (name == "hand" or sum(1 for c in carried if c > 0) >= 3)      # records cut by segment borders
        assert got == [(c, len(pl)) for c, _s, pl in bm.bgzf_walk(raw)], name


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def stubbed(pkg, monkeypatch):
    """bamindex.main with the device call replaced: the arguments it would run with"""
    bi, cli = _mod("bamindex"), _mod("cli")
    calls = []

    def fake(ctx, in_bam, out_bai=None, segment_bytes=256 << 20, n_threads=4):
        calls.append((in_bam, out_bai, n_threads))
        return dict(records=3, refs_with_records=1, chunks=2, no_coor=1)
    monkeypatch.setattr(bi, "index_bam", fake)
    monkeypatch.setattr(cli, "_context", lambda: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("SMI_ACTIVE_PROCESSORS", raising=False)
    return bi, calls


def test_command_line_argument_forms(stubbed, tmp_path, capsys):
    bi, calls = stubbed
    bam = tmp_path / "x.bam"
    bam.write_bytes(bc.hand()[0])
    assert bi.main([str(bam)]) == 0
    assert bi.main([str(bam), str(tmp_path / "other.bai")]) == 0
    assert bi.main(["-@", "3", str(bam)]) == 0
    assert bi.main(["-@8", str(bam), str(tmp_path / "o.bai")]) == 0
    assert bi.main([str(bam), "-@", "64"]) == 0
    assert [(c[0], c[1]) for c in calls] == [(str(bam), f"{bam}.bai"), (str(bam), str(tmp_path / "other.bai")), (str(bam), f"{bam}.bai"),
                                            (str(bam), str(tmp_path / "o.bai")), (str(bam), f"{bam}.bai")]
    assert [c[2] for c in calls[2:]] == [3, 8, 16]
    assert "3 records, 1 references with records, 2 chunks, 1 records without a reference" in capsys.readouterr().err
    assert bi.main([]) == 0 and "samtools index" in capsys.readouterr().out


def test_command_line_refusals(stubbed, tmp_path, capsys, monkeypatch):
    bi, calls = stubbed
    bam = tmp_path / "x.bam"
    bam.write_bytes(bc.hand()[0])
    for argv, text in (([str(tmp_path / "missing.bam")], "no such file"), ([str(bam), str(tmp_path / "nodir" / "o.bai")], "no such directory"),
                       ([str(bam), str(tmp_path)], "a directory"), (["-@", "x", str(bam)], "not a number"), (["-@"], "needs a number"),
                       (["-q", str(bam)], "unknown option"), ([str(bam), "a", "b"], "usage"), (["-@", "-2", str(bam)], "not a thread count")):
        assert bi.main(argv) == 1, argv
        assert text in capsys.readouterr().err, argv
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert bi.main([str(bam)]) == 1
    assert "start it without torchrun" in capsys.readouterr().err
    assert calls == []


def test_a_stop_is_exit_code_1_and_names_the_read(stubbed, tmp_path, capsys, monkeypatch):
    bi, _calls = stubbed
    lib = _mod("lib")

    def stop(*a, **k):
        raise lib.BamIndexError("read back (record 30): it is out of coordinate order", "back", 30)
    monkeypatch.setattr(bi, "index_bam", stop)
    bam = tmp_path / "x.bam"
    bam.write_bytes(bc.hand()[0])
    assert bi.main([str(bam)]) == 1
    err = capsys.readouterr().err
    assert "read back (record 30)" in err and f"{bam}.bai was not written" in err


def test_cli_main_still_refuses_an_index_sub_command(pkg, capsys):
    cli = _mod("cli")
    assert cli.main(["index", "x.bam"]) == 1
    assert "this build has" in capsys.readouterr().err
