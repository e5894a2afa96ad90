"""The validator of CollapseModel on the GPU against tests/validatormodel.py: all five files byte for byte, every count and the message lines,
through lib.Collapse and through collapse_model, on the hand-built case and the size, contention, table and order edges of
tests/validatorcases.py (tests/test_validator_cpu.py asserts that each edge is in its input)."""
import importlib
import io
import os

import numpy as np
import pytest

import bammodel
import collapsecases as cc
import collapsemodel as cm
import validatorcases as vc
import validatormodel as vm

pytestmark = pytest.mark.gpu
MODEL_KW = ("delta", "min_evidence", "rn_min", "max_clip")


@pytest.fixture(scope="module")
def col(pkg):
    return importlib.import_module("sicelore_amd.collapsemodel")


@pytest.fixture(scope="module")
def lib(pkg):
    return importlib.import_module("sicelore_amd.lib")


def _through_function(col, ctx, tmp_path, bam, refflat, csv, cage, polya, short, segment_bytes=256 << 20, model=None, **kw):
    """collapse_model file to file -> (info, model counts, model validator counts); files, counts and messages compared with the model
    (model: its result where a test has computed it already)"""
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bam, block=3000))
    (tmp_path / "r.refFlat").write_text(refflat)
    (tmp_path / "c.csv").write_text(csv)
    (tmp_path / "cage.bed").write_bytes(cage.encode())
    (tmp_path / "polya.bed").write_bytes(polya.encode())
    (tmp_path / "short.bam").write_bytes(bammodel.bgzf_compress(short, block=500))
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    log = io.StringIO()
    paths = dict(cage=str(tmp_path / "cage.bed"), polya=str(tmp_path / "polya.bed"), short=str(tmp_path / "short.bam"))
    info = col.collapse_model(ctx, str(tmp_path / "in.bam"), str(tmp_path / "r.refFlat"), str(tmp_path / "c.csv"), str(out), prefix="t",
                              segment_bytes=segment_bytes, n_threads=3, log=log, **paths, **kw)
    vkw = {k: v for k, v in kw.items() if k in MODEL_KW + ("cage_co", "polya_co", "junc_co", "table_log2")}
    want, cnt, v, _sup, _genes = model or vm.collapse_model(bam, refflat, csv, cage, polya, short, **vkw)
    names = col.output_names("t", kw.get("delta", 2), kw.get("rn_min", 1), kw.get("min_evidence", 2))
    assert sorted(os.listdir(out)) == sorted(names.values())
    for sfx, data in want.items():
        assert (out / names[sfx]).read_bytes() == data, sfx
    assert {k: info[k] for k in cnt} == cnt
    assert {k: info[k] for k in v} == v
    assert log.getvalue().split("\n")[:-1] == vm.message_lines(cnt, v, paths["cage"], paths["polya"])
    assert info["stage_ms"]["jsup"] >= 0 and info["seconds"]["short"] > 0
    return info, cnt, v


def _segments_of(lib, short, segment_bytes):
    """the inflated BAM cut into (bytes, records) pieces of about segment_bytes, with the reference names"""
    arr = np.frombuffer(short, dtype=np.uint8).copy()
    _text, refs, start = lib.bam_header(arr)
    recs, end = lib.bam_index_records(arr, start, cap=max(1, (arr.size - start) // 36))
    assert end == arr.size
    pieces, i = [], 0
    while i < recs.size:
        j = i + 1
        while j < recs.size and int(recs["rec_off"][j] + recs["rec_len"][j] - recs["rec_off"][i]) <= segment_bytes:
            j += 1
        lo, hi = int(recs["rec_off"][i]), int(recs["rec_off"][j - 1] + recs["rec_len"][j - 1])
        part = recs[i:j].copy()
        for f in ("rec_off", "name_off", "cigar_off", "seq_off", "qual_off", "aux_off"):
            part[f] -= lo
        pieces.append((arr[lo:hi].copy(), part))
        i = j
    return [r[0] for r in refs], pieces


def _through_handle(lib, ctx, bam, refflat, csv, cage, polya, short, segment_bytes=256 << 20, **kw):
    """lib.Collapse: run(), then the three validate calls -> (validated files, counts, validator counts, the files of run() alone)"""
    arr = np.frombuffer(bam, dtype=np.uint8).copy()
    _text, refs, start = lib.bam_header(arr)
    recs, _end = lib.bam_index_records(arr, start, cap=max(1, (arr.size - start) // 36))
    ckw = {k: v for k, v in kw.items() if k in MODEL_KW}
    vkw = {k: v for k, v in kw.items() if k in ("cage_co", "polya_co", "junc_co", "table_log2")}
    h = lib.Collapse(ctx, refflat.encode(), csv.encode(), [r[0] for r in refs], n_threads=3, **ckw)
    try:
        if recs.size:
            h.add_segment(arr, recs)
        plain = h.run()
        names, pieces = _segments_of(lib, short, segment_bytes)
        h.validate_begin(cage.encode(), polya.encode(), names, **vkw)
        for seg, part in pieces:
            h.validate_segment(seg, part)
        outs = h.validate_end()
        return outs, h.counts(), h.validate_counts(), plain, len(pieces)
    finally:
        h.close()


def _check_handle(lib, ctx, bam, refflat, csv, cage, polya, short, **kw):
    outs, counts, vcounts, plain, n_seg = _through_handle(lib, ctx, bam, refflat, csv, cage, polya, short, **kw)
    mkw = {k: v for k, v in kw.items() if k != "segment_bytes"}
    want, cnt, v, sup, _genes = vm.collapse_model(bam, refflat, csv, cage, polya, short, **mkw)
    assert outs == want
    assert {k: counts[k] for k in cnt} == cnt and vcounts == v
    assert plain == cm.collapse_model(bam, refflat, csv, **{k: v for k, v in mkw.items() if k in MODEL_KW})[0]   # run() alone: today's files
    return v, sup, n_seg


HAND = (cc.HAND_REF, cc.HAND_CSV, vc.HAND_CAGE, vc.HAND_POLYA)


@pytest.mark.parametrize("segment_bytes", [256 << 20, 700])
def test_hand_built_case(col, lib, gpu_ctx, tmp_path, segment_bytes):
    info, cnt, v = _through_function(col, gpu_ctx, tmp_path, vc.hand_bam(), *HAND, vc.hand_short(), segment_bytes=segment_bytes)
    assert v["valid_isoforms"] == 8 and v["junction_hits"] == 18 and v["short_boundaries"] == 32
    v2, sup, n_seg = _check_handle(lib, gpu_ctx, vc.hand_bam(), *HAND, vc.hand_short(), segment_bytes=segment_bytes)
    assert sup == vc.HAND_SUPPORT and (n_seg > 3) == (segment_bytes == 700)       # the counters add up across segments


@pytest.mark.parametrize("co", [dict(junc_co=3), dict(cage_co=0), dict(polya_co=0), dict(cage_co=0, polya_co=0, junc_co=3)], ids=str)
def test_hand_built_case_cut_offs(col, lib, gpu_ctx, tmp_path, co):
    info, cnt, v = _through_function(col, gpu_ctx, tmp_path, vc.hand_bam(), *HAND, vc.hand_short(), **co)
    key = (co.get("cage_co", 50), co.get("polya_co", 50), co.get("junc_co", 1))
    assert v["valid_isoforms"] == 3 + len(vc.HAND_VALID[key])
    _check_handle(lib, gpu_ctx, vc.hand_bam(), *HAND, vc.hand_short(), **co)


def test_short_dictionary_with_chrB(lib, gpu_ctx):
    v, sup, _n = _check_handle(lib, gpu_ctx, vc.hand_bam(), *HAND, vc.hand_short(True))
    assert sup[("chrB", 100, 500)] == 1 and sup[("chr12", 100, 500)] == 2 and v["junction_keys"] == 16


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_short_record_counts(col, lib, gpu_ctx, tmp_path, n):
    bam, ref, csv = vc.keys_case(3)
    v, _sup, _n = _check_handle(lib, gpu_ctx, bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, vc.short_sizes(n))
    assert v["short_records"] == n and v["junction_hits"] == n - n // 4
    if n in (0, 65):                                              # a header-only SHORT through the file-to-file function too
        _through_function(col, gpu_ctx, tmp_path, bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, vc.short_sizes(n))


def test_one_counter_under_contention(lib, gpu_ctx):
    bam, ref, csv = vc.keys_case(1)
    v, sup, _n = _check_handle(lib, gpu_ctx, bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, vc.short_for_keys(1, [10000]))
    assert sup == {("chr12",) + vc.key_junction(0): 10000} and v["junction_hits"] == 10000


def test_long_cigar(lib, gpu_ctx):
    bam, ref, csv, short, bounds = vc.long_cigar_case()
    v, sup, _n = _check_handle(lib, gpu_ctx, bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, short)
    assert v["short_boundaries"] == 120 and sup == {("chr12",) + bounds[k]: 1 for k in vc.LONG_KEYS}


def test_full_table_and_a_table_too_small(lib, gpu_ctx):
    reads = [k % 4 for k in range(64)]
    bam, ref, csv = vc.keys_case(64)
    v, sup, _n = _check_handle(lib, gpu_ctx, bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, vc.short_for_keys(64, reads), table_log2=6)
    assert v["table_slots"] == 64 == v["junction_keys"] and [sup[("chr12",) + vc.key_junction(k)] for k in range(64)] == reads
    # every slot is full: a boundary that is no key probes all 64 and stops (the sixty-fifth junction of the next case, here absent)
    short = vc.short_for_keys(65, [1] * 65)
    v, sup, _n = _check_handle(lib, gpu_ctx, bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, short, table_log2=6)
    assert v["junction_hits"] == 64 and v["short_boundaries"] == 65
    bam, ref, csv = vc.keys_case(65)
    with pytest.raises(lib.SmiError, match="64 slots does not hold the 65"):
        _through_handle(lib, gpu_ctx, bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, short, table_log2=6)
    v, _sup, _n = _check_handle(lib, gpu_ctx, bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, short)
    assert v["table_slots"] == 256 and v["junction_hits"] == 65


def test_keys_that_differ_in_one_member(lib, gpu_ctx):
    bam, ref, csv, short = vc.near_keys_case()
    v, sup, _n = _check_handle(lib, gpu_ctx, bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, short)
    assert sorted(sup.values()) == [0, 1, 1, 2]


@pytest.fixture(scope="module")
def seeded():
    bam, ref, csv = cc.seeded_case(5)
    short, _modes = vc.seeded_short(bam, ref, csv, 11)
    return bam, ref, csv, short, vm.collapse_model(bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, short)


def test_seeded_case_in_segments(col, gpu_ctx, tmp_path, seeded):
    bam, ref, csv, short, model = seeded
    files = []
    for segment_bytes in (100000, 30000):
        d = tmp_path / str(segment_bytes)
        d.mkdir()
        info, cnt, v = _through_function(col, gpu_ctx, d, bam, ref, csv, vc.FLAT_CAGE, vc.FLAT_CAGE, short, segment_bytes=segment_bytes, model=model,
                                              delta=2)
        files.append({p: (d / "out" / p).read_bytes() for p in sorted(os.listdir(d / "out"))})
        assert 0 < v["junction_hits"] < 4000 and v["short_boundaries"] == 4000 and v["short_records"] == 20000
    assert files[0] == files[1]


def test_without_the_keywords_todays_output(col, gpu_ctx, tmp_path):
    """the shared renderer: no validate call, no keyword -> the files and lines of tests/collapsemodel.py"""
    bam = vc.hand_bam()
    for k, text in (("in.bam", bammodel.bgzf_compress(bam, block=3000)), ("r.refFlat", cc.HAND_REF.encode()), ("c.csv", cc.HAND_CSV.encode()),
                    ("cage.bed", vc.HAND_CAGE.encode()), ("polya.bed", vc.HAND_POLYA.encode())):
        (tmp_path / k).write_bytes(text)
    want, cnt, _det = cm.collapse_model(bam, cc.HAND_REF, cc.HAND_CSV)
    # none of the three; two of the three; three of which one names no file
    for n, kw in enumerate((dict(), dict(cage=str(tmp_path / "cage.bed"), polya=str(tmp_path / "polya.bed")),
                            dict(cage=str(tmp_path / "cage.bed"), polya=str(tmp_path / "polya.bed"), short=str(tmp_path / "absent.bam")))):
        out = tmp_path / f"out{n}"
        out.mkdir()
        log = io.StringIO()
        info = col.collapse_model(gpu_ctx, str(tmp_path / "in.bam"), str(tmp_path / "r.refFlat"), str(tmp_path / "c.csv"), str(out), prefix="t",
                                  n_threads=3, log=log, **kw)
        for sfx, data in want.items():
            assert (out / f"t.d2.rn1.e2{sfx}").read_bytes() == data, sfx
        assert {k: info[k] for k in cnt} == cnt and "valid_isoforms" not in info and "short" not in info["seconds"]
        assert "\tWon't perform validation (please provide CAGE bed, POLYA bed and SHORT read bam files" in log.getvalue().split("\n")
        assert log.getvalue().split("\n")[:-1] == col.statistics_lines(cnt)


@pytest.mark.parametrize("which", sorted(vc.BAD_BED_LINES))
def test_bad_bed_line_fails_by_its_number(lib, gpu_ctx, which):
    no = vc.BAD_BED_LINES[which][0]
    with pytest.raises(lib.SmiError, match=f"CAGE line {no}:"):
        _through_handle(lib, gpu_ctx, vc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, vc.bad_cage(which), vc.HAND_POLYA, vc.hand_short())
    with pytest.raises(lib.SmiError, match=f"POLYA line {no}:"):
        _through_handle(lib, gpu_ctx, vc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, vc.HAND_CAGE, vc.bad_cage(which), vc.hand_short())


def test_bed_text_forms(lib, gpu_ctx):
    """the forms of tests/test_validator_cpu.py::test_bed_text_forms through the library's parser: counts and distances"""
    cage = ("chr12 1000 1010 n 1e3 +  \nchr12\t990\t1010\tn\t.\t+\nchr12\t1001\t1010\tn\tNaN\t+x\r"
            "chr12\t1002\t1010\tn\t1\t+\t5\t9\tred\r\nchr12\t1003\t1010\tn\t1\t+\t5\t9\t1,x\nchr12\t1004\t9\tn\t1\t+\t5\t9\t0\t2\t2,2,\t0,2,\n"
            "trackchr\t5\nbrowserx\t5\n#x\t5\nchr12\n\nchrZ\t5")
    v, _sup, _n = _check_handle(lib, gpu_ctx, vc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, cage, vc.HAND_POLYA, vc.hand_short())
    assert (v["cage_references"], v["cage_entries"]) == (2, 7)


def test_short_that_is_no_bam_fails_by_name(col, lib, gpu_ctx, tmp_path):
    for k, text in (("in.bam", bammodel.bgzf_compress(vc.hand_bam(), block=3000)), ("r.refFlat", cc.HAND_REF.encode()), ("c.csv", cc.HAND_CSV.encode()),
                    ("cage.bed", vc.HAND_CAGE.encode()), ("polya.bed", vc.HAND_POLYA.encode()), ("text.bam", b"@HD\tVN:1.6\n" * 40),
                    ("nobam.bam", bammodel.bgzf_compress(b"not a BAM at all" * 10))):
        (tmp_path / k).write_bytes(text)
    (tmp_path / "out").mkdir()
    for short in ("text.bam", "nobam.bam"):
        with pytest.raises(lib.SmiError, match=f"SHORT .*{short}"):
            col.collapse_model(gpu_ctx, str(tmp_path / "in.bam"), str(tmp_path / "r.refFlat"), str(tmp_path / "c.csv"), str(tmp_path / "out"),
                               cage=str(tmp_path / "cage.bed"), polya=str(tmp_path / "polya.bed"), short=str(tmp_path / short))
        assert os.listdir(tmp_path / "out") == []


def test_call_order(lib, gpu_ctx):
    arr = np.frombuffer(vc.hand_bam(), dtype=np.uint8).copy()
    _t, refs, start = lib.bam_header(arr)
    recs, _e = lib.bam_index_records(arr, start, cap=4096)
    h = lib.Collapse(gpu_ctx, cc.HAND_REF.encode(), cc.HAND_CSV.encode(), [r[0] for r in refs])
    try:
        h.add_segment(arr, recs)
        with pytest.raises(lib.SmiError, match="smi_collapse_run comes first"):
            h.validate_begin(b"", b"", ["chr12"])
        h.run()
        with pytest.raises(lib.SmiError, match="between smi_collapse_validate_begin"):
            h.validate_segment(arr, recs)
        with pytest.raises(lib.SmiError, match="smi_collapse_validate_begin comes first"):
            h.validate_end()
        h.validate_begin(b"", b"", ["chr12"])
        with pytest.raises(lib.SmiError, match="already called"):
            h.validate_begin(b"", b"", ["chr12"])
        bad = recs[:1].copy()
        bad["rec_off"] = arr.size - 10
        with pytest.raises(lib.SmiError, match="lies outside the segment"):
            h.validate_segment(arr, bad)
        h.validate_end()
        with pytest.raises(lib.SmiError, match="between smi_collapse_validate_begin"):
            h.validate_segment(arr, recs)
    finally:
        h.close()
