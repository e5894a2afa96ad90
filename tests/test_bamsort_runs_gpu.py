"""BamSort through sorted runs on the GPU (K-MERGE-RANK, K-MERGE-SLICES, K-MERGE-GATHER, smi_bamsort.hip, through bamsort.sort_bam with
runs_prefix): every case of tests/sortcases.py and of tests/runmodel.py under a budget that forces runs, the written file byte for byte
the resident sort's and its inflated bytes the model's (tests/sortmodel.py), the runs and slices the model's (tests/runmodel.py), no run
file left; the stop and the refusals; the index; and the chain with the sort as a process.  tests/test_bamsort_runs_cpu.py asserts that
each input holds the edges named here."""
import functools
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as graft
import baicases as bc
import baimodel as bm
import bammodel
import runmodel as rm
import sortcases as sc
import sortmodel as sm

pytestmark = pytest.mark.gpu
EOF = bammodel.bgzf_block(b"")
STAGES = {"key", "sort", "gather", "deflate"}
RUN_STAGES = {"spill_gather", "merge_sort", "slices", "stage_upload"}


def _mod(name):
    return importlib.import_module(f"{graft.PKG_NAME}.{name}")


@pytest.fixture(scope="module")
def bs(pkg):
    return _mod("bamsort")


@pytest.fixture(scope="module")
def lib(pkg):
    return _mod("lib")


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (raw, segment_bytes, window_bytes, the model's sorted stream, the record lengths in input order)"""
    if name == "seeded":
        raw, seg, win = sc.seeded()[0], 30_000, 64 << 10
    else:
        raw, seg, win = (rm.RUN_CASES[name] if name in rm.RUN_CASES else sc.CASES[name])()
    return raw, seg, win, sm.sorted_stream(raw), [r["length"] for r in sm.split(bammodel.bgzf_decompress(raw))[3]]


def _counts(path, seg):
    """the record counts of the segments the reader cuts the file into"""
    return [int(recs.size) for _bam, recs, _hdr in _mod("bamsegments").segments(str(path), seg, 1) if recs.size]


def _left(tmp_path):
    return sorted(f for f in os.listdir(tmp_path) if ".run" in f or ".tmp" in f)


def _through_runs(bs, ctx, tmp_path, name, budget=None, **kw):
    """the case sorted resident and through runs under `budget` (default: the least that refuses no segment): the two files are equal byte
    for byte, the inflated bytes are the model's, the runs are the model's, nothing temporary is left -> (info of the run sort, the plan)"""
    raw, seg, win, want, lengths = _case(name)
    src = tmp_path / "in.bam"
    src.write_bytes(raw)
    counts = _counts(src, seg)
    budget = budget or (rm.least_budget(lengths, counts) if lengths else 1 << 20)
    runs, n_runs, windows, slices = rm.plan(raw, counts, budget, win)
    plain = bs.sort_bam(ctx, str(src), str(tmp_path / "resident.bam"), segment_bytes=seg, window_bytes=win, n_threads=2, **kw)
    info = bs.sort_bam(ctx, str(src), str(tmp_path / "runs.bam"), segment_bytes=seg, window_bytes=win, n_threads=2, resident_bytes=budget,
                       runs_prefix=str(tmp_path / "spill"), **kw)
    written = (tmp_path / "runs.bam").read_bytes()
    assert written == (tmp_path / "resident.bam").read_bytes() and written.endswith(EOF) and info["bytes_written"] == len(written)
    assert bammodel.bgzf_decompress(written) == want
    assert _left(tmp_path) == []
    sizes = [sum(n for n, r in zip(lengths, runs) if r == j) for j in range(n_runs)]
    assert (info["runs"], info["run_bytes"], info["largest_run"]) == (n_runs, sum(sizes), max(sizes, default=0))
    assert info["records"] == plain["records"] == len(lengths) and info["windows"] == plain["windows"] == len(windows)
    assert info["segments"] == len(counts) and info["largest_window"] == plain["largest_window"]
    assert set(info["stage_ms"]) == (STAGES | RUN_STAGES if n_runs else STAGES) and set(plain["stage_ms"]) == STAGES
    assert ("run_write" in info["seconds"]) == ("run_read" in info["seconds"]) == bool(n_runs)
    return info, (runs, n_runs, windows, slices, counts, budget)


def _drive(lib, ctx, path, seg, win, budget):
    """the handle driven by hand as sort_bam drives it -> (the handle after finish, the run files' bytes, the number of windows)"""
    h, files = None, []

    def spill():
        nw, _n, size = h.spill_begin()
        files.append(b"".join(h.spill_window(k).tobytes() for k in range(nw)))
        assert len(files[-1]) == size
        h.spill_end()
    try:
        for bam, recs, hdr in _mod("bamsegments").segments(str(path), seg, 1):
            if hdr is not None:
                h = lib.BamSort(ctx, len(lib.bam_header(np.frombuffer(hdr, dtype=np.uint8))[1]), budget, win)
                h.run_mode()
            if recs.size and not h.add_segment(bam, recs):
                spill()
                assert h.add_segment(bam, recs)
        if files:
            spill()
        return h, files, h.finish()[0]
    except BaseException:
        if h is not None:
            h.close()
        raise


# ---- 1. every case, with runs where it has more than one segment ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_every_sort_case_through_runs(bs, gpu_ctx, tmp_path, name):
    info, (_runs, n_runs, _w, _s, counts, _b) = _through_runs(bs, gpu_ctx, tmp_path, name)
    assert (n_runs >= 3) == (len(counts) > 1) and (n_runs == 0) == (name in ("header_only", "one_record"))
    if name == "hand":
        assert [r["name"] for r in bammodel.parse_bam(bammodel.bgzf_decompress((tmp_path / "runs.bam").read_bytes()))[2]] == sc.HAND_ORDER
    if name == "ties":                         # the groups' members stand in input order across the run borders
        names = [r["name"] for r in bammodel.parse_bam(bammodel.bgzf_decompress((tmp_path / "runs.bam").read_bytes()))[2]]
        at = 0
        for g, n in enumerate(sc.TIE_GROUPS):
            assert names[at:at + n] == [f"t{g}_{k}" for k in range(n)]
            at += n


def test_seeded_shuffle_every_window_from_every_run(bs, gpu_ctx, tmp_path):
    info, (_runs, n_runs, windows, slices, _c, _b) = _through_runs(bs, gpu_ctx, tmp_path, "seeded")
    assert n_runs >= 4 and info["records"] == 20300 and all(all(s[1] for s in per) for per in slices)


# ---- 2. many runs, short runs, the long record, the budget's edge ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,least", [("runs_65", 65), ("runs_257", 257)])
def test_more_runs_than_a_wavefront_and_than_a_block(bs, gpu_ctx, tmp_path, name, least):
    info, (runs, n_runs, _w, _s, _c, _b) = _through_runs(bs, gpu_ctx, tmp_path, name)
    assert info["runs"] == n_runs >= least and 1 in {runs.count(j) for j in set(runs)}             # and runs of exactly one record


def test_long_record_in_a_run_and_a_window_of_its_own(bs, gpu_ctx, tmp_path):
    info, (runs, n_runs, windows, slices, _c, _b) = _through_runs(bs, gpu_ctx, tmp_path, "long_record")
    assert n_runs == 3 and runs.count(runs[rm.LONG_AT]) == 1 and info["largest_window"] == info["largest_run"] == 70000


def test_budget_exactly_full_and_one_byte_short(bs, gpu_ctx, tmp_path):
    full, _plan = _through_runs(bs, gpu_ctx, tmp_path, "exact", budget=rm.EXACT_BUDGET)
    short, _plan = _through_runs(bs, gpu_ctx, tmp_path, "exact", budget=rm.EXACT_BUDGET - 1)
    assert (full["runs"], short["runs"]) == (2, 3) and full["largest_run"] == 10100 and short["largest_run"] == 5200


# ---- 3. the slices, against the model; the host loop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hand", "ties", "alignments", "runs_65"])
def test_slices_are_the_models_and_the_run_files_are_sorted_runs(lib, gpu_ctx, tmp_path, name):
    raw, seg, win, want, lengths = _case(name)
    src = tmp_path / "in.bam"
    src.write_bytes(raw)
    counts = _counts(src, seg)
    budget = rm.least_budget(lengths, counts)
    runs, n_runs, windows, slices = rm.plan(raw, counts, budget, win)
    h, files, n_windows = _drive(lib, gpu_ctx, src, seg, win, budget)
    try:
        assert (len(files), n_windows) == (n_runs, len(windows))
        # a run file holds the run's records in the model's order
        data = bammodel.bgzf_decompress(raw)
        hdr, recs = sm.sorted_records(data)
        text, _d, refs, parsed = sm.split(data)
        for j, blob in enumerate(files):
            mine = [i for i in range(len(parsed)) if runs[i] == j]
            mine.sort(key=lambda i: sm.key(parsed[i], len(refs)))
            assert blob == b"".join(data[parsed[i]["off"]:parsed[i]["off"] + parsed[i]["length"]] for i in mine), j
        body = b""
        for k, per in enumerate(slices):
            first, size, ordinal = h.window_slices(k)
            assert [(int(a), int(b), int(c)) for a, b, c in zip(first, size, ordinal)] == [s[:3] for s in per], k
            piece = np.frombuffer(b"".join(files[j][s[0]:s[0] + s[1]] for j, s in enumerate(per)), dtype=np.uint8)
            z, inflated = h.merge_window(k, piece, inflated=True)
            assert bammodel.bgzf_decompress(z.tobytes() + EOF) == inflated.tobytes()
            body += inflated.tobytes()
        assert body == b"".join(recs) and want.endswith(body)
        # the wrong bytes' count, the resident window call and the host loop are refused by their texts
        with pytest.raises(lib.SmiError, match="takes the .* bytes of its slices"):
            h.merge_window(0, np.zeros(1, dtype=np.uint8))
        with pytest.raises(lib.SmiError, match="the records are in run files"):
            h.window(0)
        with pytest.raises(lib.SmiError, match="the host loop needs the arena, which run mode does not keep"):
            h.host_loop()
    finally:
        h.close()


# ---- 4. everything fits ------------------------------------------------------------------------------------------------------------------------
def test_a_prefix_without_need_writes_no_run(bs, gpu_ctx, tmp_path, monkeypatch):
    raw, seg, win, want, lengths = _case("ties")
    src = tmp_path / "in.bam"
    src.write_bytes(raw)
    opened = []
    real = open
    monkeypatch.setattr("builtins.open", lambda f, *a, **k: (opened.append(str(f)), real(f, *a, **k))[1])
    plain = bs.sort_bam(gpu_ctx, str(src), str(tmp_path / "a.bam"), segment_bytes=seg, window_bytes=win, n_threads=2)
    enough = sum(lengths) + rm.PER_RECORD * len(lengths)
    for budget in (None, enough):
        info = bs.sort_bam(gpu_ctx, str(src), str(tmp_path / "b.bam"), segment_bytes=seg, window_bytes=win, n_threads=2, resident_bytes=budget,
                           runs_prefix=str(tmp_path / "nodir" / "spill"))
        assert (info["runs"], info["run_bytes"], info["arena_bytes"]) == (0, 0, sum(lengths)) and set(info["stage_ms"]) == STAGES
        assert (tmp_path / "b.bam").read_bytes() == (tmp_path / "a.bam").read_bytes()
    assert plain["runs"] == 0 and not [f for f in opened if ".run" in f] and _left(tmp_path) == []
    # one byte less and there are runs; their directory is missing, which is an OSError with nothing left behind
    with pytest.raises(OSError):
        bs.sort_bam(gpu_ctx, str(src), str(tmp_path / "b2.bam"), segment_bytes=seg, window_bytes=win, n_threads=2, resident_bytes=enough - 1,
                    runs_prefix=str(tmp_path / "nodir" / "spill"))
    assert sorted(os.listdir(tmp_path)) == ["a.bam", "b.bam", "in.bam"]


# ---- 5. the index ------------------------------------------------------------------------------------------------------------------------------
def test_index_with_runs_is_the_models_and_the_resident_sorts(bs, gpu_ctx, tmp_path):
    info, (_runs, n_runs, _w, _s, _c, _b) = _through_runs(bs, gpu_ctx, tmp_path, "seeded", index=True)
    written, bai = (tmp_path / "runs.bam").read_bytes(), (tmp_path / "runs.bam.bai").read_bytes()
    assert n_runs >= 4 and info["index_error"] is None and info["index"]["records"] == 20300
    assert bai == bm.bai_model(written) and bai == (tmp_path / "resident.bam.bai").read_bytes()


# ---- 6. the stop and the refusals ----------------------------------------------------------------------------------------------------------------
def test_stop_behind_a_spill_names_the_read_and_leaves_nothing(bs, lib, gpu_ctx, tmp_path, capsys, monkeypatch):
    raw, seg, win, record, read = sc.stop()
    p, out = tmp_path / "in.bam", str(tmp_path / "out.bam")
    p.write_bytes(raw)
    data = bammodel.bgzf_decompress(raw)
    lengths = [r["length"] for r in bammodel.parse_bam(data)[2]]
    counts = _counts(p, seg)
    budget = rm.least_budget(lengths, counts)
    assert rm.run_of(lengths, counts, budget)[0][record] >= 1                          # the record lies behind the first spill
    with pytest.raises(lib.BamSortError) as plain:
        bs.sort_bam(gpu_ctx, str(p), out, n_threads=2, segment_bytes=seg, window_bytes=win)
    with pytest.raises(lib.BamSortError) as e:
        bs.sort_bam(gpu_ctx, str(p), out, n_threads=2, segment_bytes=seg, window_bytes=win, resident_bytes=budget, runs_prefix=str(tmp_path / "spill"))
    assert (e.value.record, e.value.read) == (plain.value.record, plain.value.read) == (record, read) and str(e.value) == str(plain.value)
    assert os.listdir(tmp_path) == ["in.bam"]
    monkeypatch.setattr(_mod("cli"), "_context", lambda: gpu_ctx)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    real, seen = bs.sort_bam, []

    def sized(ctx, a, b, **kw):
        seen.append(kw)
        return real(ctx, a, b, **dict(kw, segment_bytes=seg, window_bytes=win))
    monkeypatch.setattr(bs, "sort_bam", sized)
    assert bs.main(["--resident-bytes", str(budget), "-T", str(tmp_path / "sorttmp"), "--write-index", "-o", out, str(p)]) == 1
    err = capsys.readouterr().err
    assert f"read {read} (record {record})" in err and "was not written" in err
    assert seen[0]["runs_prefix"] == str(tmp_path / "sorttmp") and seen[0]["resident_bytes"] == budget
    assert os.listdir(tmp_path) == ["in.bam"]


def test_a_segment_beyond_the_budget_is_refused_by_name(bs, lib, gpu_ctx, tmp_path):
    raw, seg, win, _want, lengths = _case("ties")
    p = tmp_path / "in.bam"
    p.write_bytes(raw)
    counts = _counts(p, seg)
    budget = rm.least_budget(lengths, counts) - 1
    with pytest.raises(rm.SegmentTooLarge) as m:
        rm.run_of(lengths, counts, budget)
    assert m.value.segment >= 2                                                       # runs were written before it
    for b, sizes in ((budget, dict(segment_bytes=seg, window_bytes=win)), (sum(lengths), {})):         # and the whole file as one segment
        with pytest.raises(lib.SmiError) as e:
            bs.sort_bam(gpu_ctx, str(p), str(tmp_path / "out.bam"), resident_bytes=b, runs_prefix=str(tmp_path / "spill"), n_threads=2, **sizes)
        text = str(e.value)
        assert "BamSort: a segment of " in text and f"exceed resident_bytes = {b}" in text and "lower segment_bytes or raise resident_bytes" in text
        assert not isinstance(e.value, lib.BamSortError) and os.listdir(tmp_path) == ["in.bam"]


# ---- 7. the chain the scripts have, with runs --------------------------------------------------------------------------------------------------
def test_sort_through_runs_as_a_process_between_two_gpu_programs(bs, lib, gpu_ctx, tmp_path):
    refs, sorted_raw = bc.writer_input()
    data = bammodel.bgzf_decompress(sorted_raw)
    R = [data[r["off"]:r["off"] + r["length"]] for r in bammodel.parse_bam(data)[2]]
    np.random.default_rng(5).shuffle(R)
    raw = bammodel.bgzf_compress(bammodel.bam_bytes("@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs), refs, R),
                                 block=3000)
    src, dst = tmp_path / "molecules.bam", tmp_path / "sorted.bam"
    src.write_bytes(raw)
    budget = rm.PER_RECORD * len(R) + sum(len(r) for r in R) // 2                    # the arrays of every record and half the record bytes
    r = subprocess.run([sys.executable, os.path.join(graft.PKG_DIR, "bamsort.py"), "--resident-bytes", str(budget), "-T", str(tmp_path / "sorttmp"),
                        "--write-index", "-@", "2", "-o", str(dst), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"through (\d+) runs of (\d+) bytes", r.stderr)
    assert m and int(m.group(1)) >= 2 and int(m.group(2)) == sum(len(x) for x in R), r.stderr[-2000:]
    written = dst.read_bytes()
    assert bammodel.bgzf_decompress(written) == sm.sorted_stream(raw) and written.endswith(EOF)
    assert sorted(os.listdir(tmp_path)) == ["molecules.bam", "sorted.bam", "sorted.bam.bai"]
    assert (tmp_path / "sorted.bam.bai").read_bytes() == bm.bai_model(written)
    rf = tmp_path / "genes.refFlat"
    rf.write_text(bc.WRITER_REFFLAT)
    tagged = _mod("moltags").add_gene_name_tag(gpu_ctx, str(dst), str(tmp_path / "tagged.bam"), str(rf), n_threads=2, index=True)
    assert tagged["index_error"] is None and tagged["index"]["records"] == len(R)
    assert (tmp_path / "tagged.bam.bai").read_bytes() == bm.bai_model((tmp_path / "tagged.bam").read_bytes())
