"""BamSort on the GPU (K-SORT-KEY, K-SORT-GATHER, smi_bamsort.hip, through bamsort.sort_bam): every case of tests/sortcases.py in one
segment and one window and again in four or more segments with windows of a few kilobytes, the product's inflated bytes against the
model's (tests/sortmodel.py); the stop and the budget refusal; the index as a by-product; and the chain the scripts have, the sort between
two GPU programs.  tests/test_bamsort_cpu.py asserts that each input holds the edges named here."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as graft
import baicases as bc
import baimodel as bm
import bammodel
import sortcases as sc
import sortmodel as sm

pytestmark = pytest.mark.gpu
ONE = 256 << 20
EOF = bammodel.bgzf_block(b"")


def _mod(name):
    return importlib.import_module(f"{graft.PKG_NAME}.{name}")


@pytest.fixture(scope="module")
def bs(pkg):
    return _mod("bamsort")


@pytest.fixture(scope="module")
def lib(pkg):
    return _mod("lib")


def _clean(tmp_path):
    return not [f for f in os.listdir(tmp_path) if ".tmp" in f]


def _sort(bs, ctx, tmp_path, raw, segment_bytes=ONE, window_bytes=64 << 20, name="out.bam", **kw):
    """-> (the product's inflated bytes, info); the file ends with the end-of-file block, the model's reader reads it, no .tmp is left"""
    src, dst = tmp_path / "in.bam", tmp_path / name
    src.write_bytes(raw)
    info = bs.sort_bam(ctx, str(src), str(dst), segment_bytes=segment_bytes, window_bytes=window_bytes, n_threads=2, **kw)
    written = dst.read_bytes()
    assert written.endswith(EOF) and info["bytes_written"] == len(written) and _clean(tmp_path)
    return bammodel.bgzf_decompress(written), info


def _both(bs, ctx, tmp_path, raw, seg, win):
    """one segment and one window, and the segmented run: both equal the model -> (the model's stream, info of the segmented run)"""
    want = sm.sorted_stream(raw)
    one, info1 = _sort(bs, ctx, tmp_path, raw)
    many, info = _sort(bs, ctx, tmp_path, raw, seg, win)
    assert one == want and many == want
    _hdr, recs = sm.sorted_records(bammodel.bgzf_decompress(raw))
    lens = [len(r) for r in recs]
    assert info1["segments"] <= 1 and info1["windows"] == min(len(recs), 1) and info["windows"] == len(sm.windows(lens, win))
    assert info["records"] == info1["records"] == len(recs) and info["arena_bytes"] == sum(lens)
    return want, info


# ---- 1. the hand-built files -------------------------------------------------------------------------------------------------------------
def test_hand_built_file(bs, gpu_ctx, tmp_path):
    raw, seg, win = sc.hand()
    want, info = _both(bs, gpu_ctx, tmp_path, raw, seg, win)
    assert [r["name"] for r in bammodel.parse_bam(want)[2]] == sc.HAND_ORDER
    assert info["segments"] >= 4 and info["windows"] >= 4
    assert set(info["stage_ms"]) == {"key", "sort", "gather", "deflate"} and info["seconds"]["device"] > 0


@pytest.mark.parametrize("name", ["header_only", "one_record", "no_references", "many_references"])
def test_small_and_large_dictionaries(bs, gpu_ctx, tmp_path, name):
    raw, seg, win = sc.CASES[name]()
    _want, info = _both(bs, gpu_ctx, tmp_path, raw, seg, win)
    assert info["records"] == dict(header_only=0, one_record=1, no_references=60, many_references=2022)[name]


# ---- 2. stability ------------------------------------------------------------------------------------------------------------------------
def test_tie_groups_keep_their_input_order(bs, gpu_ctx, tmp_path):
    raw, seg, win = sc.ties()
    want, info = _both(bs, gpu_ctx, tmp_path, raw, seg, win)
    assert info["segments"] >= 4
    names = [r["name"] for r in bammodel.parse_bam(want)[2]]
    at = 0
    for g, n in enumerate(sc.TIE_GROUPS):                # (the streams are equal, so this is the product's order)
        assert names[at:at + n] == [f"t{g}_{k}" for k in range(n)]
        at += n


# ---- 3. the gather -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["alignments", "lengths"])
def test_gather_alignments_and_lengths(bs, gpu_ctx, tmp_path, name):
    """all 256 pairs of (source offset mod 16, destination offset mod 16); records of 37 .. 70,000 bytes, the window that holds only the
    long record and the window that ends exactly on its limit"""
    raw, seg, win = sc.CASES[name]()
    _want, info = _both(bs, gpu_ctx, tmp_path, raw, seg, win)
    assert info["segments"] >= 4 and info["windows"] >= 4
    if name == "lengths":
        assert info["largest_window"] == 70000


# ---- 4. orders ---------------------------------------------------------------------------------------------------------------------------
def test_sorted_input_comes_back_as_it_is(bs, gpu_ctx, tmp_path):
    raw, seg, win = sc.already_sorted()
    want, _info = _both(bs, gpu_ctx, tmp_path, raw, seg, win)
    assert want == bammodel.bgzf_decompress(raw)


def test_reversed_input(bs, gpu_ctx, tmp_path):
    raw, seg, win = sc.reversed_input()
    _both(bs, gpu_ctx, tmp_path, raw, seg, win)


@pytest.fixture(scope="module")
def seeded():
    raw, _refs = sc.seeded()
    return raw, sm.sorted_stream(raw)


def test_seeded_shuffle_in_segments_twice_and_the_host_loop(bs, lib, gpu_ctx, tmp_path, seeded):
    raw, want = seeded
    a, info_a = _sort(bs, gpu_ctx, tmp_path, raw, 100_000, 64 << 10)
    b, info_b = _sort(bs, gpu_ctx, tmp_path, raw, 30_000, 64 << 10)
    assert a == want and b == want
    assert info_a["records"] == 20300 and 4 <= info_a["segments"] < info_b["segments"] and info_a["windows"] == info_b["windows"] >= 4
    # the same sort on the host, over the bytes the device holds, against the device's windows
    h = None
    try:
        for bam, recs, hdr in _mod("bamsegments").segments(str(tmp_path / "in.bam"), 30_000, 2):
            if hdr is not None:
                h = lib.BamSort(gpu_ctx, 5, window_bytes=64 << 10)
            if recs.size:
                h.add_segment(bam, recs)
        assert h.finish() == (info_a["windows"], 20300)
        seconds, mismatches = h.host_loop()
        assert mismatches == 0 and seconds > 0
    finally:
        if h is not None:
            h.close()


# ---- 5. the stop -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segmented", [False, True])
def test_stop_names_the_read_and_leaves_nothing(bs, lib, gpu_ctx, tmp_path, capsys, monkeypatch, segmented):
    raw, seg, win, record, read = sc.stop()
    p, out = tmp_path / "in.bam", str(tmp_path / "out.bam")
    p.write_bytes(raw)
    sizes = dict(segment_bytes=seg, window_bytes=win) if segmented else {}
    with pytest.raises(lib.BamSortError) as e:
        bs.sort_bam(gpu_ctx, str(p), out, n_threads=2, **sizes)
    assert (e.value.record, e.value.read) == (record, read)
    assert f"read {read} (record {record})" in str(e.value) and "ref_id" in str(e.value)
    assert os.listdir(tmp_path) == ["in.bam"]
    # through the command line: exit code 1, the same names on stderr, still nothing written
    monkeypatch.setattr(_mod("cli"), "_context", lambda: gpu_ctx)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    real = bs.sort_bam
    monkeypatch.setattr(bs, "sort_bam", lambda ctx, a, b, **kw: real(ctx, a, b, **dict(kw, **sizes)))
    assert bs.main(["--write-index", "-o", out, str(p)]) == 1
    err = capsys.readouterr().err
    assert f"read {read} (record {record})" in err and "was not written" in err
    assert os.listdir(tmp_path) == ["in.bam"]


# ---- 6. the budget -----------------------------------------------------------------------------------------------------------------------
def test_a_bam_beyond_the_budget_is_refused_by_name(bs, lib, gpu_ctx, tmp_path):
    raw, seg, win = sc.ties()
    inflated = len(bammodel.bgzf_decompress(raw))
    p = tmp_path / "in.bam"
    p.write_bytes(raw)
    for sizes in ({}, dict(segment_bytes=seg, window_bytes=win)):
        with pytest.raises(lib.SmiError) as e:
            bs.sort_bam(gpu_ctx, str(p), str(tmp_path / "out.bam"), resident_bytes=inflated // 2, n_threads=2, **sizes)
        assert f"BamSort: the BAM inflates to more than {inflated // 2} bytes; this build sorts a BAM that is resident in device memory" in str(e.value)
        assert not isinstance(e.value, lib.BamSortError) and os.listdir(tmp_path) == ["in.bam"]
    # and with room for the records and their arrays it runs
    got, _info = _sort(bs, gpu_ctx, tmp_path, raw, resident_bytes=inflated + 48 * sum(sc.TIE_GROUPS))
    assert got == sm.sorted_stream(raw)


# ---- 7. the index ------------------------------------------------------------------------------------------------------------------------
def test_index_is_the_models_and_bamindexs(bs, gpu_ctx, tmp_path, seeded, capsys, monkeypatch):
    raw, want = seeded
    plain, info0 = _sort(bs, gpu_ctx, tmp_path, raw, 100_000, 64 << 10, name="plain.bam")
    assert "index" not in info0 and not [f for f in os.listdir(tmp_path) if f.endswith(".bai")]          # no .bai by default
    got, info = _sort(bs, gpu_ctx, tmp_path, raw, 100_000, 64 << 10, index=True)
    written = (tmp_path / "out.bam").read_bytes()
    assert got == want and written == (tmp_path / "plain.bam").read_bytes()
    bai = (tmp_path / "out.bam.bai").read_bytes()
    assert info["index_error"] is None and info["index"]["bytes_written"] == len(bai) and info["index"]["records"] == 20300
    assert bai == bm.bai_model(written)
    again = _mod("bamindex").index_bam(gpu_ctx, str(tmp_path / "out.bam"), str(tmp_path / "again.bai"), n_threads=2)
    assert again["records"] == 20300 and (tmp_path / "again.bai").read_bytes() == bai
    assert bm.uncovered(written, bai, bc.random_regions(bm.records_of(written)[0], 200)) == []
    # --write-index through main
    monkeypatch.setattr(_mod("cli"), "_context", lambda: gpu_ctx)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert bs.main(["-@", "2", "--write-index", "-o", str(tmp_path / "cl.bam"), str(tmp_path / "in.bam")]) == 0
    assert "20300 records" in capsys.readouterr().err
    assert bammodel.bgzf_decompress((tmp_path / "cl.bam").read_bytes()) == want
    assert (tmp_path / "cl.bam.bai").read_bytes() == bm.bai_model((tmp_path / "cl.bam").read_bytes()) and _clean(tmp_path)


def test_a_sorted_file_no_index_holds_keeps_its_bam(bs, gpu_ctx, tmp_path):
    """the hand-built file has a record on a reference at pos = -1: the BAM is complete, index_error says why there is no .bai"""
    raw, seg, win = sc.hand()
    got, info = _sort(bs, gpu_ctx, tmp_path, raw, seg, win, index=True)
    assert got == sm.sorted_stream(raw)
    assert info["index"] is None and "c1_minus1" in info["index_error"] and "the BAM is complete" in info["index_error"]
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".bai")]


# ---- 8. the chain the scripts have ---------------------------------------------------------------------------------------------------------
def test_sort_as_a_process_between_two_gpu_programs(bs, lib, gpu_ctx, tmp_path):
    refs, sorted_raw = bc.writer_input()
    _text, _refs, recs = bammodel.parse_bam(bammodel.bgzf_decompress(sorted_raw))
    data = bammodel.bgzf_decompress(sorted_raw)
    R = [data[r["off"]:r["off"] + r["length"]] for r in recs]
    np.random.default_rng(5).shuffle(R)
    raw = bammodel.bgzf_compress(bammodel.bam_bytes("@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs), refs, R))
    src, dst = tmp_path / "molecules.bam", tmp_path / "sorted.bam"
    src.write_bytes(raw)
    bi = _mod("bamindex")
    with pytest.raises(lib.BamIndexError):
        bi.index_bam(gpu_ctx, str(src), n_threads=2)
    r = subprocess.run([sys.executable, os.path.join(graft.PKG_DIR, "bamsort.py"), "--write-index", "-@", "2", "-o", str(dst), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    written = dst.read_bytes()
    assert bammodel.bgzf_decompress(written) == sm.sorted_stream(raw) and written.endswith(EOF) and _clean(tmp_path)
    assert (tmp_path / "sorted.bam.bai").read_bytes() == bm.bai_model(written)
    info = bi.index_bam(gpu_ctx, str(dst), str(tmp_path / "own.bai"), n_threads=2)
    assert info["records"] == len(R) and (tmp_path / "own.bai").read_bytes() == (tmp_path / "sorted.bam.bai").read_bytes()
    rf = tmp_path / "genes.refFlat"
    rf.write_text(bc.WRITER_REFFLAT)
    tagged = _mod("moltags").add_gene_name_tag(gpu_ctx, str(dst), str(tmp_path / "tagged.bam"), str(rf), n_threads=2, index=True)
    assert tagged["index_error"] is None and tagged["index"]["records"] == len(R)
    assert (tmp_path / "tagged.bam.bai").read_bytes() == bm.bai_model((tmp_path / "tagged.bam").read_bytes())
