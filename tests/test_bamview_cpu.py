"""BamView without a GPU: the model (tests/viewmodel.py) on a file written out by hand, the region grammar, the index reader against
baimodel's, the ranges a query reads, bamsegments.ranges against the full scan, the command line with the device call stubbed, and the
edges tests/test_bamview_gpu.py claims, asserted as properties of the inputs (tests/viewcases.py)."""
import importlib
import struct

import pytest

import __graft_entry__ as graft
import baicases as bc
import baimodel as bm
import bammodel
import viewcases as vc
import viewmodel as vm


def _mod(name):
    return importlib.import_module(f"{graft.PKG_NAME}.{name}")


@pytest.fixture(scope="module")
def bv(pkg):
    return _mod("bamview")


@pytest.fixture(scope="module")
def built():
    """every case once: name -> (raw, segment_bytes, regions as the case has them, as triples, filters, (our index, the foreign one) or None)"""
    out = {}
    for name, make in vc.CASES.items():
        raw, seg, regions, filters = make()
        out[name] = (raw, seg, regions, vc.regions_of(raw, regions), filters, vc.indexes(raw) if regions is not None else None)
    return out


def _names(raw):
    return [r["name"] for r in bammodel.parse_bam(bammodel.bgzf_decompress(raw))[2]]


def _kept(raw, regions, filters):
    names = _names(raw)
    return [names[k] for k in vm.scan(raw, regions, **filters)[2]]


# ---- 1. the model ---------------------------------------------------------------------------------------------------------------------------
def test_model_on_the_file_written_out_by_hand():
    raw, _seg, regions, filters = vc.hand()
    trip = vc.regions_of(raw, regions)
    assert trip == [(0, 100, 110), (1, 16, 1 << 29)]
    assert _kept(raw, trip, filters) == ["a", "b", "d", "e"]
    assert _kept(raw, [(0, 110, 20000)], {}) == [] and _kept(raw, [(0, 109, 20001)], {}) == ["a", "c"]
    assert _kept(raw, [(0, 106, 107)], {}) == ["a"]                      # b is flag 0x4: one base, whatever its CIGAR says
    assert _kept(raw, None, dict(exclude=4)) == ["a", "c", "d", "e"] and _kept(raw, None, dict(require=16)) == ["d"]
    assert _kept(raw, None, dict(min_mapq=30)) == ["a", "b", "d", "e", "u"]
    data = bammodel.bgzf_decompress(raw)
    out = vm.view(raw, trip)
    assert out[:50] == data[:50] and len(out) == len(data) - len(vc.rec("c", 0, 20000, [("M", 5)], mapq=5)) - len(bc.unplaced("u"))
    assert bammodel.parse_bam(out)[0] == bc.HEAD + "@SQ\tSN:chr1\tLN:100000\n@SQ\tSN:chr2\tLN:1000\n"


# ---- 2. regions -----------------------------------------------------------------------------------------------------------------------------
NAMES = ["chr1", "HLA:A", "chr1:5", "dup", "dup", "x"]


@pytest.mark.parametrize("text,want", [("chr1", (0, 0, 1 << 29)), ("chr1:10", (0, 9, 1 << 29)), ("chr1:10-20", (0, 9, 20)), ("chr1:1,000-2,000,000", (0, 999, 2000000)),
                                       ("chr1:5", (2, 0, 1 << 29)), ("chr1:5:7-9", (2, 6, 9)), ("HLA:A", (1, 0, 1 << 29)), ("HLA:A:3", (1, 2, 1 << 29)),
                                       ("dup:4-4", (3, 3, 4)), ("x:1-999999999999", (5, 0, 1 << 29)), ("x:600000000", (5, 599999999, 1 << 29))])
def test_parse_region_forms(bv, text, want):
    assert bv.parse_region(text, NAMES) == want == vm.parse_region(text, NAMES)


@pytest.mark.parametrize("text,kind,says", [("chr9", "name", "is not one of the header's references"), ("chr9:1-5", "name", "'chr9' is not one of the header's references"),
                                            ("HLA:B", "name", "'HLA' is not one of the header's references"), ("chr1:0", "beg", "BEG is below 1"),
                                            ("chr1:0-5", "beg", "BEG is below 1"), ("chr1:10-9", "end", "END is below BEG"), ("chr1:", "number", "is not a number"),
                                            ("chr1:5-", "number", "'' is not a number"), ("chr1:-5", "number", "is not a number"), ("chr1:1e3", "number", "'1e3' is not a number"),
                                            ("chr1:5-7-9", "number", "'7-9' is not a number"), ("chr1:,", "number", "is not a number"), ("chr1:١", "number", "is not a number"),
                                            ("", "name", "is not one of")])
def test_parse_region_refusals(bv, text, kind, says):
    with pytest.raises(vm.RegionStop) as m:
        vm.parse_region(text, NAMES)
    assert m.value.kind == kind
    with pytest.raises(bv.ViewStop, match=says.replace("'", ".")):
        bv.parse_region(text, NAMES)


def test_tuples_and_merging(bv):
    got = bv.resolve_regions([("x", 5, 9), (0, 0, 1 << 40), "dup:2"], NAMES)
    assert got == [(5, 5, 9), (0, 0, 1 << 29), (3, 1, 1 << 29)]
    for bad, says in ((("nope", 0, 5), "is not one of"), ((9, 0, 5), "reference 9"), ((0, -1, 5), "BEG is below 1"), ((0, 9, 5), "END is below BEG")):
        with pytest.raises(bv.ViewStop, match=says):
            bv.resolve_regions([bad], NAMES)
    R = [(1, 5, 9), (0, 150, 300), (0, 100, 200), (0, 300, 400), (0, 401, 402), (0, 7, 7), (1, 5, 9)]
    assert bv.merge_regions(R) == [(0, 100, 400), (0, 401, 402), (1, 5, 9)] == vm.merged(R)


# ---- 3. the index ---------------------------------------------------------------------------------------------------------------------------
def test_read_bai_equals_the_models_reader(bv, built):
    files = {name: ix for name, (_r, _s, _g, _t, _f, ix) in built.items() if ix is not None}
    files["baicases.chunks"] = vc.indexes(bc.chunks()[0])
    files["baicases.linear"] = vc.indexes(bc.linear()[0])
    for name, (ours, foreign) in files.items():
        assert bv.read_bai(ours) == bm.parse_bai(ours), name
        assert bv.read_bai(foreign) == bm.parse_bai(foreign), name
        assert bv.read_bai(foreign)[1] is None and all(r["meta"] is None for r in bv.read_bai(foreign)[0]), name
        assert all(b < 4681 for r in bv.read_bai(foreign)[0] for b in r["bins"]), name
    ours = files["hand"][0]
    for cut, says in ((ours[:len(ours) - 3], "bytes behind its last entry"), (ours[:30], "ends inside an entry"), (b"BAM\1" + ours[4:], "does not begin with BAI"),
                      (ours + b"\0", "bytes behind its last entry")):
        with pytest.raises(bv.ViewStop, match=says):
            bv.read_bai(cut)


def test_foreign_index_covers_every_record(built):
    for name in ("borders", "intervals", "many_references"):
        raw, _seg, _regions, trip, _filters, (_ours, foreign) = built[name]
        assert bm.uncovered(raw, foreign, trip) == [], name
    raw = bc.linear()[0]
    assert bm.uncovered(raw, vc.indexes(raw)[1], bc.random_regions([("chr1", bc.BIG)], n=50)) == []


def _inside(raw, rngs, kept):
    mine = set(vm.seen(raw, rngs))
    return all(k in mine for k in kept)


def test_query_ranges_are_merged_disjoint_and_cover(bv, built):
    for name, (raw, _seg, _regions, trip, filters, ix) in built.items():
        if ix is None:
            continue
        refs = bammodel.parse_bam(bammodel.bgzf_decompress(raw))[1]
        for k, bai in enumerate(ix):
            parsed = bv.read_bai(bai)
            rngs = bv.query_ranges(parsed, bv.merge_regions(trip))
            assert rngs == vm.ranges(bai, trip), (name, k)
            assert all(b < e for b, e in rngs) and all(a[1] < b[0] for a, b in zip(rngs, rngs[1:])), (name, k)
            assert _inside(raw, rngs, vm.scan(raw, trip)[2]), (name, k)
            if len(refs) < 10:
                for region in bc.random_regions([(n, min(ln, 1 << 20)) for n, ln in refs], n=200, seed=13):
                    one = bv.query_ranges(parsed, bv.merge_regions([region]))
                    assert one == vm.ranges(bai, [region]) and _inside(raw, one, vm.scan(raw, [region])[2]), (name, k, region)


def test_last_window_stands_for_the_windows_behind_it(bv):
    """a region that begins behind the linear index's windows reads what lies behind the last window's value, as baimodel.bai_query does"""
    raw = bc.file_of([("chr1", 1 << 29)], [vc.rec("a", 0, 100), vc.rec("long", 0, 200, [("M", 5), ("N", 1 << 20), ("M", 5)]), vc.rec("b", 0, 300)], block=100)
    for bai in vc.indexes(raw):
        rngs = bv.query_ranges(bv.read_bai(bai), [(0, 1 << 19, (1 << 19) + 5)])
        assert rngs == vm.ranges(bai, [(0, 1 << 19, (1 << 19) + 5)]) and _inside(raw, rngs, [1])


# ---- 4. the reader of ranges ------------------------------------------------------------------------------------------------------------------
def _read(pkg, tmp_path, raw, rngs, segment_bytes):
    seg = _mod("bamsegments")
    p = tmp_path / "r.bam"
    p.write_bytes(raw)
    stats, out, n_seg = {}, [], 0
    for bam, recs in seg.ranges(str(p), rngs, segment_bytes, 2, stats=stats):
        n_seg += 1
        assert recs.size
        out += [bam[int(r["rec_off"]):int(r["rec_off"]) + int(r["rec_len"])].tobytes() for r in recs]
        assert all(bam[int(r["name_off"]) + int(r["l_read_name"]) - 1] == 0 for r in recs)
    return out, stats, n_seg


def _range_file():
    """blocks cut so that record 3 straddles two blocks and record 10 straddles two; record 6 ends at a block's end"""
    H = bc.header([("chr1", 1 << 20)])
    R = [vc.rec(f"r{k}", 0, 100 * k, aux=b"XZZ" + bytes(65 + (k * j) % 23 for j in range(40 + 7 * k)) + b"\0") for k in range(16)]
    at = [len(H)]
    for r in R:
        at.append(at[-1] + len(r))
    cuts = [at[1], at[3] + 20, at[7], at[10] + 9, at[13]]
    return bc.cut_blocks(H + b"".join(R), cuts), R, at


def test_ranges_reader_against_the_full_scan(pkg, tmp_path):
    raw, R, _at = _range_file()
    _refs, recs = bm.records_of(raw)
    v = [(r[4], r[5]) for r in recs]
    cases = {"mid-block begin, block end": (v[4][0], v[6][1]), "straddling record at the begin": (v[3][0], v[5][1]), "straddling record at the end": (v[8][0], v[10][1]),
             "whole blocks": (v[1][0], v[6][1]), "one record": (v[9][0], v[9][1]), "everything": (v[0][0], v[15][1])}
    assert v[6][1] & 0xFFFF == 0 and v[4][0] & 0xFFFF and v[3][0] >> 16 != (v[3][1] - 1) >> 16 and v[10][0] >> 16 != (v[10][1] - 1) >> 16
    for name, (vb, ve) in cases.items():
        want = [R[k] for k in vm.seen(raw, [(vb, ve)])]
        for seg in (1 << 20, 1):
            got, stats, _n = _read(pkg, tmp_path, raw, [(vb, ve)], seg)
            assert got == want and want, (name, seg)
            assert (stats["blocks_read"], stats["compressed_bytes_read"]) == vm.blocks_under(raw, [(vb, ve)]), (name, seg)
    several = [(v[1][0], v[2][1]), (v[4][0], v[4][1]), (v[6][0], v[6][1]), (v[8][0], v[11][1]), (v[14][0], v[15][1])]
    want = [R[k] for k in (1, 2, 4, 6, 8, 9, 10, 11, 14, 15)]
    assert v[4][1] >> 16 == v[6][0] >> 16 and v[4][1] & 0xFFFF                # records 4 and 6 share a block: it is read once
    assert vm.blocks_under(raw, several)[0] < sum(vm.blocks_under(raw, [r])[0] for r in several)
    got, stats, n_seg = _read(pkg, tmp_path, raw, several, 1 << 20)
    assert got == want and n_seg == 1 and (stats["blocks_read"], stats["compressed_bytes_read"]) == vm.blocks_under(raw, several)
    got, _stats, n_seg = _read(pkg, tmp_path, raw, several, 1)
    assert got == want and n_seg >= 4


def test_ranges_leave_in_file_order_whatever_the_batching(pkg, tmp_path):
    """two ranges that wait for their neighbours, then one that begins in the block the second ended in and goes on into the next block:
    its first block's records must not leave ahead of the waiting ranges.  Every segment size from one block's to the whole file's."""
    raw, R, _at = _range_file()
    _refs, recs = bm.records_of(raw)
    v = [(r[4], r[5]) for r in recs]
    shape = [(v[1][0], v[2][1]), (v[4][0], v[4][1]), (v[6][0], v[8][1])]
    assert v[4][1] >> 16 == v[6][0] >> 16 and v[8][0] >> 16 > v[6][0] >> 16        # r6 begins in r4's block, r8 lies in the next one
    more = [(v[0][0], v[0][1]), (v[2][0], v[2][1]), (v[4][0], v[5][1]), (v[6][0], v[11][1]), (v[12][0], v[12][1]), (v[13][0], v[15][1])]
    sizes = sorted({b[1] for b in bm.bgzf_walk(raw)})
    for rngs, want in ((shape, (1, 2, 4, 6, 7, 8)), (more, (0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15))):
        for seg in [1, 1 << 20] + sizes + [2 * sizes[-1], 3 * sizes[-1], sizes[0] + sizes[-1]]:
            got, stats, n_seg = _read(pkg, tmp_path, raw, rngs, seg)
            assert got == [R[k] for k in want], (rngs, seg)
            assert (stats["blocks_read"], stats["compressed_bytes_read"]) == vm.blocks_under(raw, rngs), (rngs, seg)
    assert _read(pkg, tmp_path, raw, shape, 1 << 20)[2] == 1 and _read(pkg, tmp_path, raw, more, 1 << 20)[2] == 1


def test_a_range_cut_over_several_segments(pkg, tmp_path):
    raw = vc.lengths()[0]
    _refs, recs = bm.records_of(raw)
    data = bammodel.bgzf_decompress(raw)
    parsed = bammodel.parse_bam(data)[2]
    want = [data[r["off"]:r["off"] + r["length"]] for r in parsed]
    got, stats, n_seg = _read(pkg, tmp_path, raw, [(recs[0][4], recs[-1][5])], 3000)
    assert got == want and n_seg >= 3 and stats["blocks_read"] >= 30      # (a piece that ends inside the long record yields nothing)
    assert (stats["blocks_read"], stats["compressed_bytes_read"]) == vm.blocks_under(raw, [(recs[0][4], recs[-1][5])])


def test_ranges_that_are_no_records_stop_by_name(pkg, tmp_path):
    seg = _mod("bamsegments")
    raw, _R, _at = _range_file()
    _refs, recs = bm.records_of(raw)
    v = [(r[4], r[5]) for r in recs]
    short = bc.cut_blocks(bc.header([("chr1", 1000)]) + struct.pack("<I", 31) + bytes(31), [])
    hdr_len = len(bc.header([("chr1", 1000)]))
    for what, file, rng, says in (("mid-record begin", raw, (v[4][0] + 5, v[6][1]), "runs past the range's end|inconsistent record|shorter than"),
                                  ("end inside a record", raw, (v[4][0], v[5][1] - 3), "runs past the range's end"),
                                  ("offset outside the file", raw, (v[4][0], (len(raw) + 10) << 16), "outside the file"),
                                  ("no block there", raw, ((v[4][0] >> 16) + 1 << 16, v[6][1]), "no BGZF block|BGZF"),
                                  ("block_size below 32", short, (hdr_len, len(short) - 28 << 16), "shorter than its fixed part")):
        p = tmp_path / "bad.bam"
        p.write_bytes(file)
        with pytest.raises(seg.RangeError, match=says):
            list(seg.ranges(str(p), [rng], 1 << 20, 1))


# ---- 5. the command line --------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def stubbed(pkg, monkeypatch):
    """bamview.main with the device call replaced: the arguments it would run with"""
    bv, cli = _mod("bamview"), _mod("cli")
    calls = []

    def fake(ctx, in_bam, out_bam, regions=(), require=0, exclude=0, min_mapq=0, index=False, n_threads=4, **kw):
        calls.append((in_bam, out_bam, list(regions), require, exclude, min_mapq, index, n_threads))
        return dict(records=9, kept=5, segments=1, ranges=2, blocks_read=3, bytes_written=400)
    monkeypatch.setattr(bv, "view_bam", fake)
    monkeypatch.setattr(cli, "_context", lambda: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("SMI_ACTIVE_PROCESSORS", raising=False)
    return bv, calls


def test_command_line_argument_forms(stubbed, tmp_path, capsys):
    bv, calls = stubbed
    bam, out = tmp_path / "x.bam", str(tmp_path / "y.bam")
    bam.write_bytes(vc.hand()[0])
    x = str(bam)
    assert bv.main(["-Sb", x, "chr1", "-o", out]) == 0                      # main.nf:143 as it stands
    assert calls[-1][:7] == (x, out, ["chr1"], 0, 0, 0, False)
    assert bv.main(["-b", "-h", "-S", "-@", "3", "-f", "0x10", "-F", "1796", "-q", "20", "--write-index", "-o", out, x, "chr1:5-9", "chr2"]) == 0
    assert calls[-1] == (x, out, ["chr1:5-9", "chr2"], 16, 1796, 20, True, 3)
    assert bv.main(["-bhSq7", "-f3", "-F0X900", "-@8", "-o" + out, x]) == 0
    assert calls[-1] == (x, out, [], 3, 0x900, 7, False, 8)
    assert bv.main(["-O", "BAM", "--threads", "64", "--output", out, x]) == 0 and calls[-1][7] == 16
    assert "5 of 9 records kept in 1 segments, 2 ranges and 3 blocks read, 400 bytes written" in capsys.readouterr().err
    n = len(calls)
    assert bv.main(["-H", x]) == 0
    assert capsys.readouterr().out == bc.HEAD + "@SQ\tSN:chr1\tLN:100000\n@SQ\tSN:chr2\tLN:1000\n"
    assert bv.main(["-H", "-o", str(tmp_path / "h.txt"), x]) == 0 and capsys.readouterr().out == ""
    assert (tmp_path / "h.txt").read_text() == bc.HEAD + "@SQ\tSN:chr1\tLN:100000\n@SQ\tSN:chr2\tLN:1000\n" and len(calls) == n
    assert bv.header_text(x).count("@SQ") == 2
    assert bv.main(["-c", "-F", "4", x, "chr1"]) == 0
    assert capsys.readouterr().out == "5\n" and calls[-1][:7] == (x, None, ["chr1"], 0, 4, 0, False)
    assert bv.main([]) == 0
    text = capsys.readouterr().out
    assert "main.nf:143" in text and "have no effect" in text


def test_command_line_refusals(stubbed, tmp_path, capsys, monkeypatch):
    bv, calls = stubbed
    bam, sam, out = tmp_path / "x.bam", tmp_path / "x.sam", str(tmp_path / "y.bam")
    bam.write_bytes(vc.hand()[0])
    sam.write_text("@HD\tVN:1.6\n")
    x = str(bam)
    cases = [(["-S", "-o", out, x], "this build writes BAM alone"), (["-b", x], "writes a file, not the standard output"), (["-b", "-o", out, str(sam)], "not a BAM"),
             (["-b", "-o", out, "-"], "not the standard input"), (["-b", "-O", "sam", "-o", out, x], "-O sam: this build writes BAM alone"),
             (["-O", "cram", "-o", out, x], "writes BAM alone"), (["-b", "-o", out, str(tmp_path / "missing.bam")], "no such file"),
             (["-b", "-o", str(tmp_path / "nodir" / "y.bam"), x], "no such directory"), (["-b", "-o", str(tmp_path), x], "a directory"),
             (["-b", "-@", "x", "-o", out, x], "not a number"), (["-b", "-f", "0x", "-o", out, x], "not a number"), (["-b", "-q", "0x10", "-o", out, x], "not a number"),
             (["-b", "-q", "256", "-o", out, x], "not a MAPQ"), (["-b", "-f", "65536", "-o", out, x], "not flag bits"), (["-b", "-x", "-o", out, x], "unknown option"),
             (["-b", "--fast", "-o", out, x], "unknown option"), (["-b", "-o", out], "usage"), (["-b", "-o"], "needs a value"), (["-b", x, "-f"], "needs a value")]
    cases += [([f"-b{c}", "-o", out, x], f"-{c}: ") for c in "LrRsdD1uUMX"]
    for argv, text in cases:
        assert bv.main(argv) == 1, argv
        assert text in capsys.readouterr().err, argv
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert bv.main(["-b", "-o", out, x]) == 1
    assert "start it without torchrun" in capsys.readouterr().err
    assert calls == []


def test_a_stop_is_exit_code_1_with_its_text(stubbed, tmp_path, capsys, monkeypatch):
    bv, _calls = stubbed
    lib = _mod("lib")
    bam, out = tmp_path / "x.bam", str(tmp_path / "y.bam")
    bam.write_bytes(vc.hand()[0])
    stops = [lib.BamViewError("read beyond (record 25): its ref_id is not one of the header's references", "beyond", 25),
             bv.ViewStop("BamView: a region needs an index: neither A nor B exists (bamindex.py writes one)")]
    for e in stops:
        def stop(*a, _e=e, **k):
            raise _e
        monkeypatch.setattr(bv, "view_bam", stop)
        assert bv.main(["-b", "-o", out, str(bam), "chr1"]) == 1
        err = capsys.readouterr().err
        assert str(e) in err and f"{out} was not written" in err


def test_missing_index_and_unknown_region_stop_before_anything_is_written(bv, tmp_path):
    """(the index and the regions are looked at before the device is: no Context is needed to get here)"""
    bam, out = tmp_path / "x.bam", tmp_path / "y.bam"
    bam.write_bytes(vc.hand()[0])
    with pytest.raises(bv.ViewStop) as m:
        bv.view_bam(None, str(bam), str(out), ["chr1"])
    assert str(m.value) == f"BamView: a region needs an index: neither {bam}.bai nor {tmp_path / 'x'}.bai exists (bamindex.py writes one)"
    with pytest.raises(bv.ViewStop, match="chr7"):
        bv.view_bam(None, str(bam), str(out), ["chr7:1-5"])
    (tmp_path / "x.bai").write_bytes(vc.indexes(vc.borders()[0])[0])             # an index of another file: one reference, not two
    with pytest.raises(bv.ViewStop, match="has 1 references, the header of .* has 2: the index does not belong to the BAM"):
        bv.view_bam(None, str(bam), str(out), ["chr1"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["x.bai", "x.bam"]
    assert bv.index_path_of(str(bam)) == str(tmp_path / "x.bai")


def test_cli_main_still_does_not_know_view_and_samview_still_refuses_bam(pkg, tmp_path, capsys):
    cli = _mod("cli")
    assert cli.main(["view", "-b", "x.bam", "chr1"]) == 1
    assert "this build has" in capsys.readouterr().err
    bam = tmp_path / "x.bam"
    bam.write_bytes(vc.hand()[0])
    assert _mod("samview").main(["-b", "-o", str(tmp_path / "y.bam"), str(bam)]) == 1
    assert "this build reads SAM text" in capsys.readouterr().err


def test_library_mirror_lists_the_new_entry_points(pkg):
    lib = _mod("lib")
    names = [n for n in lib.EXPORTS if n.startswith("smi_bamview_")]
    assert sorted(names) == sorted(f"smi_bamview_{w}" for w in ("create", "add_segment", "convert", "counts", "stage_ms", "error_read", "free", "host_loop"))
    assert lib.BAMVIEW_COUNTS == ("records", "kept", "bytes", "bytes_kept", "regions", "segments") and lib.BAMVIEW_STAGES == ("test", "scan", "gather", "deflate")
    assert issubclass(lib.BamViewError, lib.SmiError)


# ---- 6. the edges the GPU file claims ---------------------------------------------------------------------------------------------------------
def test_border_case(built):
    raw, _seg, _regions, trip, filters, _ix = built["borders"]
    recs = {r["name"]: r for r in bammodel.parse_bam(bammodel.bgzf_decompress(raw))[2]}
    assert [len(recs[f"ops{n}"]["cigar"]) for n in vc.CIGAR_COUNTS] == list(vc.CIGAR_COUNTS)
    assert {op for r in recs.values() for op, _n in r["cigar"]} == set("MIDNSHP=X")
    kept = set(_kept(raw, trip, filters))
    assert bm.extent(recs["ends_at_beg"]) == (4990, 5000) and "ends_at_beg" not in kept
    assert bm.extent(recs["one_base_in"]) == (4991, 5001) and "one_base_in" in kept
    assert recs["last_base"]["pos0"] == 5999 and "last_base" in kept and recs["at_end"]["pos0"] == 6000 and "at_end" not in kept
    assert recs["flag4_long"]["flag"] & 4 and bm.extent(recs["flag4_long"]) == (4800, 4801) and "flag4_long" not in kept
    assert bm.extent(recs["SI_before"]) == (4999, 5000) and "SI_before" not in kept and "SI_first_base" in kept
    assert "across" in kept and "inside" in kept and 4 < len(kept) < len(recs) // 2


def test_interval_case(built):
    raw, _seg, _regions, trip, filters, _ix = built["intervals"]
    per_ref = {}
    for ref, _b, _e in vm.merged(trip):
        per_ref[ref] = per_ref.get(ref, 0) + 1
    assert [per_ref[k] for k in range(6)] == list(vc.INTERVAL_COUNTS)
    kept = _kept(raw, trip, filters)
    assert len(kept) == sum(vc.INTERVAL_COUNTS) and all("_in" in n for n in kept)
    assert sum("_gap" in n or "_front" in n for n in _names(raw)) == sum(vc.INTERVAL_COUNTS) + 6


def test_merging_and_reference_cases(built):
    raw, _seg, _regions, trip, filters, _ix = built["merging"]
    assert vm.merged(trip) == [(0, 100, 400), (0, 1000, 1100)] and len(trip) == 5
    assert _kept(raw, trip, filters) == ["first", "seam", "both", "second"]
    assert sum(vm.overlaps(r, [t]) for r in bammodel.parse_bam(bammodel.bgzf_decompress(raw))[2] if r["name"] == "both" for t in vm.merged(trip)) == 2
    raw, _seg, _regions, trip, filters, _ix = built["many_references"]
    assert [t[0] for t in trip] == [0, 2999, 2] and _kept(raw, trip, filters) == ["first_ref", "last_ref_b"]
    assert not any(r["ref_id"] == 2 for r in bammodel.parse_bam(bammodel.bgzf_decompress(raw))[2])
    assert _kept(*[built["nothing"][k] for k in (0, 3, 4)]) == [] and _kept(*[built["everything"][k] for k in (0, 3, 4)]) == _names(built["everything"][0])


def test_gather_cases(built):
    raw, _seg, _regions, _trip, filters, _ix = built["alignments"]
    _header, kept, idx, recs = vm.scan(raw, None, **filters)
    first, pairs, to = recs[0]["off"], set(), 0
    for k in idx:
        pairs.add(((recs[k]["off"] - first) % 16, to % 16))
        to += recs[k]["length"]
    assert len(pairs) == 256 and 1500 < len(idx) < 2500
    raw, _seg, _regions, trip, filters, _ix = built["lengths"]
    _header, kept, idx, recs = vm.scan(raw, trip, **filters)
    assert [len(b) for b in kept] == list(vc.LENGTHS) and sorted(r["length"] for r in recs) == sorted(vc.LENGTHS * 2)


def test_filter_case(built):
    raw, _seg, _regions, trip, filters, _ix = built["filters"]
    assert filters == dict(require=0x3, exclude=0x900, min_mapq=20)
    recs = {r["name"]: r for r in bammodel.parse_bam(bammodel.bgzf_decompress(raw))[2]}
    kept = _kept(raw, trip, filters)
    assert kept[:4] == ["keep", "keep_more_bits", "mapq_at", "mapq_255"] and len(kept) == 4 + 50
    assert (recs["bit1_missing"]["flag"], recs["bit2_missing"]["flag"]) == (2, 1) and recs["excluded_0x100"]["flag"] == 0x103 and recs["excluded_0x800"]["flag"] == 0x803
    assert (recs["mapq_at"]["mapq"], recs["mapq_below"]["mapq"]) == (20, 19)
    assert "outside" not in kept and vm.passes(recs["outside"], **filters)
    raw, _seg, regions, _trip, filters, ix = built["unsorted_no_region"]
    recs = bammodel.parse_bam(bammodel.bgzf_decompress(raw))[2]
    assert regions is None and ix is None and any(r["ref_id"] < 0 for r in recs) and [r["pos0"] for r in recs] != sorted(r["pos0"] for r in recs)
    assert 0 < len(_kept(raw, None, filters)) < len(recs)


def test_seeded_input_reads_less_than_the_file():
    raw, regions = vc.seeded()
    ours, foreign = vc.indexes(raw)
    assert bm.uncovered(raw, foreign, regions[:100]) == []
    for bai in (ours, foreign):
        one = vm.ranges(bai, [(2, 0, 1 << 29)])
        n_blocks, size = vm.blocks_under(raw, one)
        assert 0 < size < len(raw) // 3 and 0 < n_blocks < len(bm.bgzf_walk(raw)) // 3
    _header, kept, _idx, recs = vm.scan(raw, [(2, 0, 1 << 29)])
    assert len(kept) == sum(r["ref_id"] == 2 for r in recs) > 3000
    assert 100 < len(vm.scan(raw, regions)[1]) < len(recs) and len(vm.merged(regions)) > 500
