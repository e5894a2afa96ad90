"""BamSort's runs without a GPU: the model of the runs and the slices (tests/runmodel.py) on a case written out by hand, bamsort.py's
command line around runs_prefix with the device call stubbed, and the edges tests/test_bamsort_runs_gpu.py claims, asserted with the
model on its inputs and budgets (conditions of the inputs, not measurements)."""
import functools
import importlib
import inspect
import os
from collections import Counter

import pytest

import __graft_entry__ as graft
import bammodel
import runmodel as rm
import sortcases as sc
import sortmodel as sm


def _mod(name):
    return importlib.import_module(f"{graft.PKG_NAME}.{name}")


@pytest.fixture(scope="module")
def lib(pkg):
    graft.build()
    return _mod("lib")


def _segments(tmp_path, raw, segment_bytes):
    """the record counts of the segments the reader cuts `raw` into"""
    p = tmp_path / "seg.bam"
    p.write_bytes(raw)
    return [int(recs.size) for _bam, recs, _hdr in _mod("bamsegments").segments(str(p), segment_bytes, 1) if recs.size]


def _lengths(raw):
    return [r["length"] for r in sm.split(bammodel.bgzf_decompress(raw))[3]]


@functools.lru_cache(maxsize=None)
def _case(name):
    return (rm.RUN_CASES[name] if name in rm.RUN_CASES else sc.CASES[name])()


def _plan(lib, tmp_path, name, budget=None, seg=None, win=None):
    """-> (lengths, segment counts, budget, runs, n_runs, windows, slices) of a case at its least budget (or `budget`)"""
    raw, seg0, win0 = _case(name)
    lengths, counts = _lengths(raw), _segments(tmp_path, raw, seg or seg0)
    budget = budget or rm.least_budget(lengths, counts)
    return (lengths, counts, budget) + rm.plan(raw, counts, budget, win or win0)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_model_on_six_records_in_three_runs():
    """input order a50 b10 | c30 d10 | e20 f40 (name and position on one reference; a and b are 60 bytes, the others 48), two records per
    segment; resident_bytes = 384: the first segment takes 120 + 96, the second would make 120 + 96 + 192 = 408, the third stands at
    96 + 288 = 384 alone.  Sorted: b d e c f a (b before d: equal keys keep the input's order); windows of 110 bytes: b d | e c | f a."""
    R = [sc.rec("a" * 13, 0, 50), sc.rec("b" * 13, 0, 10), sc.rec("c", 0, 30), sc.rec("d", 0, 10), sc.rec("e", 0, 20), sc.rec("f", 0, 40)]
    lengths = [len(r) for r in R]
    assert lengths == [60, 60, 48, 48, 48, 48]
    assert rm.run_of(lengths, [2, 2, 2], 384) == ([0, 0, 1, 1, 2, 2], 3)
    assert rm.run_of(lengths, [2, 2, 2], 600) == ([0] * 6, 0)                       # 312 + 288: everything fits
    assert rm.run_of(lengths, [2, 2, 2], 599)[1] == 2
    with pytest.raises(rm.SegmentTooLarge) as e:
        rm.run_of(lengths, [2, 2, 2], 383)
    assert e.value.segment == 2
    assert rm.least_budget(lengths, [2, 2, 2]) == 384
    raw = sc.file_of([("chr1", 1000)], R)
    runs, n_runs, windows, slices = rm.plan(raw, [2, 2, 2], 384, 110)
    assert (runs, n_runs) == ([0, 0, 1, 1, 2, 2], 3)
    assert windows == [(0, 2, 108), (2, 4, 96), (4, 6, 108)]
    # per run: (first byte in the run file, bytes, first ordinal, records); run files: b a | d c | e f
    assert slices == [[(0, 60, 0, 1), (0, 48, 2, 1), (0, 0, 4, 0)],
                      [(60, 0, 1, 0), (48, 48, 3, 1), (0, 48, 4, 1)],
                      [(60, 60, 1, 1), (96, 0, 4, 0), (48, 48, 5, 1)]]
    assert rm.stage_residues(slices) == {0, 60 % 16, 48 % 16}
    assert rm.plan(raw, [2, 2, 2], 600, 110) == ([0] * 6, 0, windows, None)
    assert [r["name"][0] for r in bammodel.parse_bam(sm.sorted_stream(raw))[2]] == list("bdecfa")


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def stubbed(pkg, monkeypatch):
    """bamsort.main with the device call replaced: the keywords it would run with"""
    bs, cli = _mod("bamsort"), _mod("cli")
    calls = []

    def fake(ctx, in_bam, out_bam, **kw):
        calls.append(kw)
        return dict(records=6, segments=3, windows=3, bytes_written=300, runs=kw.get("resident_bytes") and 3, run_bytes=312)
    monkeypatch.setattr(bs, "sort_bam", fake)
    monkeypatch.setattr(cli, "_context", lambda: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("SMI_ACTIVE_PROCESSORS", raising=False)
    return bs, calls


def test_command_line_passes_the_prefix_and_the_budget(stubbed, tmp_path, capsys):
    bs, calls = stubbed
    bam, out = tmp_path / "x.bam", str(tmp_path / "y.bam")
    bam.write_bytes(sc.one_record()[0])
    assert bs.main(["-T", str(tmp_path / "sorttmp"), "-o", out, str(bam)]) == 0
    assert bs.main(["-T" + str(tmp_path / "glued"), "-o", out, str(bam)]) == 0
    assert bs.main(["-o", out, str(bam)]) == 0
    assert "6 records in 3 segments, 3 windows, 300 bytes written\n" in capsys.readouterr().err           # no word about runs without any
    assert bs.main(["--resident-bytes", "4096", "-m", "1G", "-l", "3", "-o", out, str(bam)]) == 0
    assert "300 bytes written, through 3 runs of 312 bytes" in capsys.readouterr().err
    assert [c["runs_prefix"] for c in calls] == [str(tmp_path / "sorttmp"), str(tmp_path / "glued"), f"{out}.tmp{os.getpid()}", f"{out}.tmp{os.getpid()}"]
    assert [c["resident_bytes"] for c in calls] == [None, None, None, 4096]
    # a prefix in a directory that is not there is no argument error: it is looked at when a run is written
    assert bs.main(["-T", str(tmp_path / "nodir" / "p"), "-o", out, str(bam)]) == 0
    for value, text in (("4k", "not a number"), ("", "not a number"), ("0", "not a number of bytes"), ("-5", "not a number of bytes")):
        assert bs.main(["--resident-bytes", value, "-o", out, str(bam)]) == 1
        assert text in capsys.readouterr().err
    assert bs.main(["-o", out, str(bam), "--resident-bytes"]) == 1 and "needs a value" in capsys.readouterr().err
    assert bs.main(["-o", out, str(bam), "-T"]) == 1 and "needs a value" in capsys.readouterr().err
    assert len(calls) == 5


def test_help_text_and_the_keyword(pkg, capsys):
    bs = _mod("bamsort")
    assert bs.main(["--help"]) == 0
    text = capsys.readouterr().out
    assert "have no effect" in text and "-T PREFIX" in text and "--resident-bytes N" in text and "PREFIX.0000.run" in text and "2^31 - 1" in text
    assert "-T" not in bs.NO_EFFECT and set(bs.NO_EFFECT) == {"-m", "-l"} and "--resident-bytes" in bs.USAGE
    assert inspect.signature(bs.sort_bam).parameters["runs_prefix"].default is None
    lib = _mod("lib")
    assert lib.BAMSORT_COUNTS[-3:] == ("runs", "run_bytes", "largest_run") and lib.BAMSORT_COUNTS[:7] == ("records", "segments", "windows", "arena_bytes",
                                                                                                        "arena_held", "largest_window", "bytes_out")
    assert lib.BAMSORT_STAGES == ("key", "sort", "gather", "deflate", "spill_gather", "merge_sort", "slices", "stage_upload")


# ---- the edges the GPU test claims are in its inputs ---------------------------------------------------------------------------------------
def test_every_sort_case_spills_where_it_has_segments(lib, tmp_path):
    for name in sc.CASES:
        raw, _seg, _win = _case(name)
        lengths, counts, budget, runs, n_runs, windows, slices = _plan(lib, tmp_path, name)
        if len(counts) > 1:
            assert n_runs >= 3 and budget < sum(lengths) + rm.PER_RECORD * len(lengths), name
            assert len(windows) >= 4 and len(slices) == len(windows), name
        else:
            assert n_runs == 0 and slices is None and name in ("header_only", "one_record"), name
        with_room = rm.run_of(lengths, counts, sum(lengths) + rm.PER_RECORD * len(lengths))
        assert with_room[1] == 0, name


def test_more_runs_than_a_wavefront_and_than_a_block(lib, tmp_path):
    for name, least in (("runs_65", 65), ("runs_257", 257)):
        lengths, counts, _budget, runs, n_runs, windows, slices = _plan(lib, tmp_path, name)
        assert max(counts) == 1 and len(counts) == len(lengths)                      # one record per segment
        assert n_runs >= least and len(windows) >= 4, (name, n_runs)
        sizes = Counter(Counter(runs).values())
        assert sizes[1] >= 10 and max(sizes) >= 2                                    # runs of exactly one record, and longer ones
        assert any(sum(1 for s in per if s[1]) >= 2 for per in slices) and any(s[1] == 0 for per in slices for s in per)


def test_sorted_and_reversed_input_have_empty_and_single_run_slices(lib, tmp_path):
    for name in ("already_sorted", "reversed_input"):
        _l, _c, _b, _runs, n_runs, _windows, slices = _plan(lib, tmp_path, name)
        assert n_runs >= 3
        assert all(any(s[1] == 0 for s in per) for per in slices)                    # every window leaves some run out
        assert sum(1 for per in slices if sum(1 for s in per if s[1]) == 1) >= 4     # windows drawn from a single run


def test_seeded_case_draws_every_window_from_every_run(lib, tmp_path):
    raw, _refs = sc.seeded()
    lengths, counts = _lengths(raw), _segments(tmp_path, raw, 30_000)
    budget = rm.least_budget(lengths, counts)
    _runs, n_runs, windows, slices = rm.plan(raw, counts, budget, 64 << 10)
    assert n_runs >= 4 and len(windows) >= 4
    assert all(all(s[1] for s in per) for per in slices)
    assert len(rm.stage_residues(slices)) == 16


def test_tie_groups_lie_on_both_sides_of_a_run_border(lib, tmp_path):
    raw, _seg, _win = _case("ties")
    _l, _c, _b, runs, n_runs, _w, _s = _plan(lib, tmp_path, "ties")
    _t, _d, refs, recs = sm.split(bammodel.bgzf_decompress(raw))
    groups = {}
    for i, r in enumerate(recs):
        groups.setdefault(sm.key(r, len(refs)), []).append(i)
    spread = {len(g): len({runs[i] for i in g}) for g in groups.values()}
    assert n_runs >= 3 and set(spread) == set(sc.TIE_GROUPS)
    assert all(spread[n] >= 2 for n in (2, 63, 64, 65, 1000)) and spread[1000] == n_runs


def test_alignment_case_slices_begin_at_every_residue(lib, tmp_path):
    _l, _c, _b, _runs, n_runs, _w, slices = _plan(lib, tmp_path, "alignments")
    assert n_runs >= 4 and rm.stage_residues(slices) == set(range(16))
    assert len({s[0] % 16 for per in slices for s in per if s[1]}) == 16             # and at every residue in the run files


def test_long_record_is_a_run_and_a_window_of_its_own(lib, tmp_path):
    lengths, counts, _b, runs, n_runs, windows, slices = _plan(lib, tmp_path, "long_record")
    assert lengths[rm.LONG_AT] == 70000 == sc.LENGTHS[-1] and max(counts) == 1
    assert n_runs == 3 and Counter(runs)[runs[rm.LONG_AT]] == 1
    k = [w[2] for w in windows].index(70000)
    assert windows[k][1] - windows[k][0] == 1 and 70000 > _case("long_record")[2]
    assert [s[1] for s in slices[k]] == [0, 70000, 0]


def test_budget_exactly_full_and_one_byte_short(lib, tmp_path):
    raw, seg, _win = _case("exact")
    lengths, counts = _lengths(raw), _segments(tmp_path, raw, seg)
    assert lengths == [5200, 5000, 5100] and counts == [1, 1, 1]
    assert rm.exact_hits(lengths, counts, rm.EXACT_BUDGET) == [2]
    assert rm.run_of(lengths, counts, rm.EXACT_BUDGET) == ([0, 1, 1], 2)
    assert rm.run_of(lengths, counts, rm.EXACT_BUDGET - 1) == ([0, 1, 2], 3)
    # and the refusal: the first segment alone needs 5,200 + 48, more than either of the others
    assert rm.least_budget(lengths, counts) == 5248
    with pytest.raises(rm.SegmentTooLarge):
        rm.run_of(lengths, counts, 5247)
