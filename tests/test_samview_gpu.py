"""SamView on the GPU (K-SAM-SIZE, K-SAM-WRITE, smi_samview.hip, through samview.sam_to_bam): every case of tests/samcases.py in one segment
and again in small segments, the product's inflated bytes against the model's (tests/sammodel.py); every stop by its line and its text;
the host loop; the index as a by-product; and the chain the scripts have, view | sort | a GPU program.  tests/test_samview_cpu.py asserts
that each input holds the edges named here."""
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
import samcases as sc
import sammodel as sm
import sortmodel

pytestmark = pytest.mark.gpu
ONE = 256 << 20
EOF = bammodel.bgzf_block(b"")


def _mod(name):
    return importlib.import_module(f"{graft.PKG_NAME}.{name}")


@pytest.fixture(scope="module")
def sv(pkg):
    return _mod("samview")


@pytest.fixture(scope="module")
def lib(pkg):
    return _mod("lib")


def _clean(tmp_path):
    return not [f for f in os.listdir(tmp_path) if ".tmp" in f]


def _convert(sv, ctx, tmp_path, raw, segment_bytes=ONE, name="out.bam", **kw):
    """-> (the product's inflated bytes, info); the file ends with the end-of-file block, the model's reader reads it, no .tmp is left"""
    src, dst = tmp_path / "in.sam", tmp_path / name
    src.write_bytes(raw)
    info = sv.sam_to_bam(ctx, str(src), str(dst), segment_bytes=segment_bytes, n_threads=2, **kw)
    written = dst.read_bytes()
    assert written.endswith(EOF) and info["bytes_written"] == len(written) and _clean(tmp_path)
    return bammodel.bgzf_decompress(written), info


# ---- 1. every case, in one segment and in small ones ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_case_equals_the_model(sv, gpu_ctx, tmp_path, name):
    raw, seg = sc.CASES[name]()
    header, recs = sm.convert(raw)
    want = header + b"".join(recs)
    one, info1 = _convert(sv, gpu_ctx, tmp_path, raw)
    many, info = _convert(sv, gpu_ctx, tmp_path, raw, seg)
    assert one == want and many == want
    assert info1["segments"] == min(len(recs), 1) and info["records"] == info1["records"] == len(recs)
    assert info["record_bytes"] == sum(len(r) for r in recs) and info["references"] == len(bammodel.parse_bam(header)[1])
    if name in ("hand", "seq_lengths", "attributes"):
        assert info["segments"] >= 3
    if name == "cigars":                                   # the line of 65,535 operations is many times its segment
        assert info["segments"] == 2
    assert set(info["stage_ms"]) == {"index", "size", "scan", "write", "deflate"}


def test_standard_input_is_read_the_same_way(sv, tmp_path):
    raw, _seg = sc.hand()
    (tmp_path / "in.sam").write_bytes(raw)
    with open(tmp_path / "in.sam", "rb") as f:
        r = subprocess.run([sys.executable, os.path.join(graft.PKG_DIR, "samview.py"), "-bS", "-o", str(tmp_path / "out.bam"), "-"], stdin=f, capture_output=True,
                           text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "5 records in 1 segments" in r.stderr
    assert bammodel.bgzf_decompress((tmp_path / "out.bam").read_bytes()) == sm.stream(raw) and _clean(tmp_path)


# ---- 2. the stops --------------------------------------------------------------------------------------------------------------------------
def test_every_stop_names_its_line_and_leaves_nothing(sv, lib, gpu_ctx, tmp_path):
    p, out = tmp_path / "in.sam", str(tmp_path / "out.bam")
    for name, (raw, line, reason) in sorted(sc.stops().items()):
        p.write_bytes(raw)
        with pytest.raises(lib.SamViewError) as e:
            sv.sam_to_bam(gpu_ctx, str(p), out, n_threads=2)
        assert (e.value.line, e.value.reason) == (line, reason), name
        assert str(e.value) == f"line {line}: {reason}" and os.listdir(tmp_path) == ["in.sam"], name


def test_first_of_two_bad_lines_is_named(sv, lib, gpu_ctx, tmp_path):
    raw, line, reason = sc.two_bad_lines()
    (tmp_path / "in.sam").write_bytes(raw)
    with pytest.raises(lib.SamViewError) as e:
        sv.sam_to_bam(gpu_ctx, str(tmp_path / "in.sam"), str(tmp_path / "out.bam"), n_threads=2)
    assert (e.value.line, e.value.reason) == (line, reason) and os.listdir(tmp_path) == ["in.sam"]


def test_stop_in_a_later_segment_leaves_no_file(sv, lib, gpu_ctx, tmp_path, capsys, monkeypatch):
    raw, seg, line, reason = sc.late_stop()
    p, out = tmp_path / "in.sam", str(tmp_path / "out.bam")
    p.write_bytes(raw)
    with pytest.raises(lib.SamViewError) as e:
        sv.sam_to_bam(gpu_ctx, str(p), out, segment_bytes=seg, n_threads=2)
    assert (e.value.line, e.value.reason) == (line, reason) and os.listdir(tmp_path) == ["in.sam"]
    # through the command line: exit code 1, the line on stderr, still nothing written
    monkeypatch.setattr(_mod("cli"), "_context", lambda: gpu_ctx)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    real = sv.sam_to_bam
    monkeypatch.setattr(sv, "sam_to_bam", lambda ctx, a, b, **kw: real(ctx, a, b, **dict(kw, segment_bytes=seg)))
    assert sv.main(["-Sb", str(p), "-o", out]) == 1
    err = capsys.readouterr().err
    assert f"line {line}: {reason}" in err and "was not written" in err and os.listdir(tmp_path) == ["in.sam"]


# ---- 3. the seeded lines and the host loop -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    raw = sc.seeded()
    return raw, sm.stream(raw)


def test_seeded_lines_in_segments_and_the_host_loop(sv, lib, gpu_ctx, tmp_path, seeded):
    raw, want = seeded
    got, info = _convert(sv, gpu_ctx, tmp_path, raw, 2_000_000)
    assert got == want and info["records"] == sc.SEEDED_LINES and info["segments"] >= 4 and info["seconds"]["device"] > 0
    # the same conversion on the host, segment by segment, against the device's records
    h = None
    try:
        with open(tmp_path / "in.sam", "rb") as f:
            pieces = sv.text_segments(f, 3_000_000)
            h = lib.SamView(gpu_ctx, next(pieces))
            n = 0
            for piece in pieces:
                h.add_segment(piece)
                h.convert()
                seconds, mismatches = h.host_loop()
                assert mismatches == 0 and seconds > 0
                n += 1
        assert n >= 3 and h.counts()["records"] == sc.SEEDED_LINES
    finally:
        if h is not None:
            h.close()


# ---- 4. the index --------------------------------------------------------------------------------------------------------------------------
def test_index_of_ordered_input_is_the_models(sv, gpu_ctx, tmp_path):
    raw = sc.seeded(3000, seed=5, ordered=True)
    plain, info0 = _convert(sv, gpu_ctx, tmp_path, raw, 200_000, name="plain.bam")
    assert "index" not in info0 and not [f for f in os.listdir(tmp_path) if f.endswith(".bai")]
    got, info = _convert(sv, gpu_ctx, tmp_path, raw, 200_000, index=True)
    written = (tmp_path / "out.bam").read_bytes()
    assert got == plain == sm.stream(raw) and written == (tmp_path / "plain.bam").read_bytes()
    bai = (tmp_path / "out.bam.bai").read_bytes()
    assert info["index_error"] is None and info["index"]["records"] == 3000 and info["index"]["bytes_written"] == len(bai)
    assert bai == bm.bai_model(written)


def test_unordered_input_keeps_its_bam_and_says_why_there_is_no_index(sv, gpu_ctx, tmp_path, seeded):
    raw, want = seeded
    got, info = _convert(sv, gpu_ctx, tmp_path, raw, 2_000_000, index=True)
    assert got == want and info["index"] is None and "the BAM is complete" in info["index_error"]
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".bai")]


# ---- 5. the chain the scripts have ---------------------------------------------------------------------------------------------------------
def test_view_sort_and_a_gpu_program_as_processes(gpu_ctx, tmp_path):
    refs, sorted_raw = bc.writer_input()
    data = bammodel.bgzf_decompress(sorted_raw)
    _text, _refs, recs = bammodel.parse_bam(data)
    order = np.random.default_rng(5).permutation(len(recs))
    header_text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
    shuffled = bammodel.bgzf_compress(bammodel.bam_bytes(header_text, refs, [data[recs[k]["off"]:recs[k]["off"] + recs[k]["length"]] for k in order]))
    sam, unsorted, dst = tmp_path / "x.sam", tmp_path / "unsorted.bam", tmp_path / "sorted.bam"
    sam.write_bytes(sm.sam_text(header_text, refs, [recs[k] for k in order]))
    for argv in (["samview.py", "-Sb", str(sam), "-o", str(unsorted)], ["bamsort.py", "--write-index", "-@", "2", "-o", str(dst), str(unsorted)]):
        r = subprocess.run([sys.executable, os.path.join(graft.PKG_DIR, argv[0]), *argv[1:]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
    written = dst.read_bytes()
    assert written.endswith(EOF) and _clean(tmp_path) and (tmp_path / "sorted.bam.bai").read_bytes() == bm.bai_model(written)
    rf = tmp_path / "genes.refFlat"
    rf.write_text(bc.WRITER_REFFLAT)
    tagged = _mod("moltags").add_gene_name_tag(gpu_ctx, str(dst), str(tmp_path / "tagged.bam"), str(rf), n_threads=2, index=True)
    assert tagged["index_error"] is None and tagged["index"]["records"] == len(recs)
    # the same bytes as the sort of the original BAM, bin set aside (bam_record fixes it to 4680; the mate fields are -1, -1, 0 in both)
    mine, direct = bammodel.bgzf_decompress(written), sortmodel.sorted_stream(shuffled)
    a, b = bammodel.parse_bam(mine)[2], bammodel.parse_bam(direct)[2]
    assert len(a) == len(b) == len(recs) and mine[:a[0]["off"]] == direct[:b[0]["off"]]
    for x, y in zip(a, b):
        p, q = mine[x["off"]:x["off"] + x["length"]], direct[y["off"]:y["off"] + y["length"]]
        assert p[:14] == q[:14] and p[16:] == q[16:] and q[14:16] == b"\x48\x12"
