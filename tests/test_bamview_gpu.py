"""BamView on the GPU (K-VIEW-TEST, K-VIEW-GATHER, smi_bamview.hip, through bamview.view_bam): every case of tests/viewcases.py in one
segment and again in small ones, read through this build's index and through the foreign-form one, the product's inflated bytes against
the model's full scan (tests/viewmodel.py), which uses no index; the seeded file; the host loop; every stop; the index as a by-product;
and the chain of sicelore-nf/main.nf 117 to 156 as processes.  tests/test_bamview_cpu.py asserts that each input holds the edges named
there."""
import importlib
import os
import subprocess
import sys

import pytest

import __graft_entry__ as graft
import baimodel as bm
import bammodel
import viewcases as vc
import viewmodel as vm

pytestmark = pytest.mark.gpu
ONE = 256 << 20
EOF = bammodel.bgzf_block(b"")
COUNTS = ("records", "kept", "bytes", "bytes_kept", "regions")


def _mod(name):
    return importlib.import_module(f"{graft.PKG_NAME}.{name}")


@pytest.fixture(scope="module")
def bv(pkg):
    return _mod("bamview")


@pytest.fixture(scope="module")
def lib(pkg):
    return _mod("lib")


@pytest.fixture(scope="module")
def seeded():
    raw, regions = vc.seeded()
    return raw, regions, vc.indexes(raw)


def _clean(tmp_path):
    return not [f for f in os.listdir(tmp_path) if ".tmp" in f]


def _put(tmp_path, raw, bai=None, name="in.bam"):
    src = tmp_path / name
    src.write_bytes(raw)
    if bai is not None:
        (tmp_path / f"{name}.bai").write_bytes(bai)
    elif (tmp_path / f"{name}.bai").exists():
        os.remove(tmp_path / f"{name}.bai")
    return str(src)


def _view(bv, ctx, tmp_path, raw, bai, regions, filters, segment_bytes=ONE, name="out.bam", **kw):
    """-> (the product's inflated bytes, info, the file's bytes); the file ends with the end-of-file block and no .tmp is left"""
    src, dst = _put(tmp_path, raw, bai), tmp_path / name
    info = bv.view_bam(ctx, src, str(dst), regions or (), segment_bytes=segment_bytes, n_threads=2, **filters, **kw)
    written = dst.read_bytes()
    assert written.endswith(EOF) and info["bytes_written"] == len(written) and _clean(tmp_path)
    return bammodel.bgzf_decompress(written), info, written


def _check(raw, bai, trip, filters, out, info, what):
    assert out == vm.view(raw, trip, **filters), what
    want = vm.counts(raw, bai, trip, **filters)
    assert {k: info[k] for k in COUNTS} == want, what
    if trip is None:
        assert (info["ranges"], info["blocks_read"], info["compressed_bytes_read"]) == (0, len(bm.bgzf_walk(raw)), len(raw)), what
    else:
        rngs = vm.ranges(bai, trip)
        assert (info["ranges"], info["blocks_read"], info["compressed_bytes_read"]) == (len(rngs),) + vm.blocks_under(raw, rngs), what


# ---- 1. every case: one segment and small ones, both index forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_case_equals_the_model(bv, gpu_ctx, tmp_path, name):
    raw, seg, regions, filters = vc.CASES[name]()
    trip = vc.regions_of(raw, regions)
    for form, bai in enumerate(vc.indexes(raw) if regions is not None else (None,)):
        out, info, _w = _view(bv, gpu_ctx, tmp_path, raw, bai, regions, filters)
        _check(raw, bai, trip, filters, out, info, (name, form, "one segment"))
        assert info["segments"] == (1 if info["records"] else 0) and not os.path.exists(tmp_path / "out.bam.bai")
        out, info, _w = _view(bv, gpu_ctx, tmp_path, raw, bai, regions, filters, segment_bytes=seg)
        _check(raw, bai, trip, filters, out, info, (name, form, "segmented"))
        if info["bytes"] > 8 * seg:
            assert info["segments"] > 1, (name, form)


# ---- 2. the seeded file ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one reference", "1,000 regions"])
def test_seeded(bv, gpu_ctx, tmp_path, seeded, which):
    """both index forms, each in one segment (blocks of 64 KiB: the 1,000 regions give many ranges per block, all in one launch) and in
    segments of 100,000 and of 30,000 bytes; the model's figures are worked out once per index form"""
    raw, regions, forms = seeded
    trip = [(2, 0, 1 << 29)] if which == "one reference" else regions
    asked = ["chr3"] if which == "one reference" else regions
    want = vm.view(raw, trip)
    for form, bai in enumerate(forms):
        rngs = vm.ranges(bai, trip)
        figures = dict(vm.counts(raw, bai, trip), ranges=len(rngs))
        figures["blocks_read"], figures["compressed_bytes_read"] = vm.blocks_under(raw, rngs)
        if which == "1,000 regions":
            per_block = {}
            for vb, _ve in rngs:
                per_block[vb >> 16] = per_block.get(vb >> 16, 0) + 1
            assert max(per_block.values()) >= 5 and len(rngs) > 2 * figures["blocks_read"]      # several ranges per block
        for seg in (ONE, 100_000, 30_000):
            out, info, written = _view(bv, gpu_ctx, tmp_path, raw, bai, asked, {}, segment_bytes=seg, index=True)
            assert out == want, (which, form, seg)
            assert {k: info[k] for k in figures} == figures, (which, form, seg)
            assert info["index_error"] is None and (tmp_path / "out.bam.bai").read_bytes() == bm.bai_model(written), (which, form, seg)
            assert info["segments"] == 1 if seg == ONE else info["segments"] > 1 or info["compressed_bytes_read"] <= seg, (which, form, seg)
            if which == "one reference":
                assert 0 < info["compressed_bytes_read"] < len(raw) // 3 and info["kept"] == info["records"]


def test_host_loop_agrees_with_the_device(bv, lib, gpu_ctx, tmp_path, seeded):
    raw, regions, (ours, _foreign) = seeded
    seg = _mod("bamsegments")
    src = _put(tmp_path, raw)
    merged = bv.merge_regions(regions)
    h = lib.BamView(gpu_ctx, 5, merged, exclude=4)
    try:
        n = 0
        for bam, recs in seg.ranges(src, bv.query_ranges(bv.read_bai(ours), merged), 30_000, 2):
            h.add_segment(bam, recs)
            h.convert()
            seconds, bad = h.host_loop()
            assert bad == 0 and seconds > 0
            n += 1
        assert n > 2 and h.counts()["kept"] == vm.counts(raw, ours, regions, exclude=4)["kept"] > 100
    finally:
        h.close()
    h = lib.BamView(gpu_ctx, 5, (), require=0, exclude=4, min_mapq=30)
    try:
        for bam, recs, _hdr in seg.segments(src, ONE, 2):
            h.add_segment(bam, recs)
            h.convert()
            assert h.host_loop()[1] == 0
        assert h.counts()["kept"] == vm.counts(raw, None, None, exclude=4, min_mapq=30)["kept"]
    finally:
        h.close()


# ---- 3. stops ----------------------------------------------------------------------------------------------------------------------------------
def _stop_index(raw):
    """an index a reader reaches the bad records through: they are filed on chr1 where they stand"""
    _refs, recs = bm.records_of(raw)
    return bammodel.bai_bytes(2, [(0, max(r[1], 0), max(r[2], 1), r[4], r[5]) for r in recs])


def test_ref_id_outside_the_header_stops_the_run(bv, lib, gpu_ctx, tmp_path, capsys):
    raw, seg, record, read = vc.stop_ref()
    for bai, regions in ((None, ()), (_stop_index(raw), ["chr1"])):
        src, dst = _put(tmp_path, raw, bai), tmp_path / "out.bam"
        for segment_bytes in (ONE, seg):
            with pytest.raises(lib.BamViewError) as m:
                bv.view_bam(gpu_ctx, src, str(dst), regions, segment_bytes=segment_bytes, n_threads=2)
            assert (m.value.read, m.value.record) == (read, record) and f"read {read} (record {record})" in str(m.value)
            assert not dst.exists() and _clean(tmp_path)
        assert bv.main(["-b", "-o", str(dst), src] + list(regions)) == 1
        err = capsys.readouterr().err
        assert f"read {read} (record {record}): its ref_id is not one of the header's references" in err and "was not written" in err
        assert not dst.exists() and _clean(tmp_path)


def test_index_stops(bv, gpu_ctx, tmp_path, capsys):
    raw, _seg, regions, _filters = vc.borders()
    other = vc.indexes(vc.hand()[0])[0]                                           # two references, not one
    dst = tmp_path / "out.bam"
    for bai, says in ((None, "a region needs an index: neither"), (other, "has 2 references, the header of"), (vc.mid_record_index(raw), "does not belong to")):
        src = _put(tmp_path, raw, bai)
        with pytest.raises(bv.ViewStop, match=says):
            bv.view_bam(gpu_ctx, src, str(dst), ["chr1"], n_threads=2)
        assert not dst.exists() and _clean(tmp_path)
        assert bv.main(["-b", "-o", str(dst), src, "chr1"]) == 1
        err = capsys.readouterr().err
        assert says in err and "was not written" in err and not dst.exists() and _clean(tmp_path)
    src = _put(tmp_path, raw, vc.mid_record_index(raw))
    assert bv.view_bam(gpu_ctx, src, str(dst), ["chr1"], index_path=_put(tmp_path, vc.indexes(raw)[1], name="elsewhere.bai"), n_threads=2)["kept"] > 100


# ---- 4. the index as a by-product ----------------------------------------------------------------------------------------------------------------
def test_write_index(bv, gpu_ctx, tmp_path, seeded, capsys):
    raw, _regions, (ours, _foreign) = seeded
    bamindex = _mod("bamindex")
    _out, _info, plain = _view(bv, gpu_ctx, tmp_path, raw, ours, ["chr2", "chr4:1-20,000,000"], dict(exclude=4), segment_bytes=100_000)
    assert not (tmp_path / "out.bam.bai").exists()
    _out, info, with_index = _view(bv, gpu_ctx, tmp_path, raw, ours, ["chr2", "chr4:1-20,000,000"], dict(exclude=4), segment_bytes=100_000, name="ix.bam", index=True)
    assert with_index == plain and info["index_error"] is None and info["index"]["records"] == info["kept"]
    left = (tmp_path / "ix.bam.bai").read_bytes()
    assert left == bm.bai_model(with_index)
    bamindex.index_bam(gpu_ctx, str(tmp_path / "ix.bam"), str(tmp_path / "again.bai"), n_threads=2)
    assert (tmp_path / "again.bai").read_bytes() == left
    src = _put(tmp_path, raw, ours)
    assert bv.main(["-b", "--write-index", "-F", "4", "-o", str(tmp_path / "cli.bam"), src, "chr2", "chr4:1-20,000,000"]) == 0
    assert "DONE" in capsys.readouterr().err and (tmp_path / "cli.bam.bai").read_bytes() == bm.bai_model((tmp_path / "cli.bam").read_bytes())
    assert bammodel.bgzf_decompress((tmp_path / "cli.bam").read_bytes()) == bammodel.bgzf_decompress(plain)


# ---- 5. processes --------------------------------------------------------------------------------------------------------------------------------
def _run(script, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(graft.PKG_DIR, script), *map(str, args)], env=env, capture_output=True, text=True, timeout=300)


def test_header_and_count_as_processes(tmp_path):
    raw, _seg, regions, _filters = vc.hand()
    src = _put(tmp_path, raw, vc.indexes(raw)[0])
    p = _run("bamview.py", "-H", src)
    assert p.returncode == 0 and p.stdout == bammodel.parse_bam(bammodel.bgzf_decompress(raw))[0], p.stderr
    p = _run("bamview.py", "-c", src, *regions)
    assert (p.returncode, p.stdout) == (0, "4\n"), p.stderr
    assert sorted(os.listdir(tmp_path)) == ["in.bam", "in.bam.bai"]


def test_the_chain_of_main_nf_as_processes(gpu_ctx, tmp_path):
    """main.nf:117 samtools index, :129 samtools view -H | grep SQ, :143-144 samtools view -Sb $bam $chromo -o chromosome.bam and its index"""
    bamindex = _mod("bamindex")
    raw, refs = vc.three_chromosomes()
    src = _put(tmp_path, raw)
    p = _run("bamindex.py", src)
    assert p.returncode == 0 and (tmp_path / "in.bam.bai").read_bytes() == bm.bai_model(raw), p.stderr
    p = _run("bamview.py", "-H", src)
    names = [f[3:] for line in p.stdout.splitlines() if line.startswith("@SQ") for f in line.split("\t") if f.startswith("SN:")]
    assert p.returncode == 0 and names == [n for n, _l in refs], p.stderr
    data = bammodel.bgzf_decompress(raw)
    _text, _refs, recs = bammodel.parse_bam(data)
    got = []
    for name in names:
        out = tmp_path / name / "chromosome.bam"
        os.mkdir(tmp_path / name)
        p = _run("bamview.py", "-Sb", src, name, "-o", out, "--write-index")
        assert p.returncode == 0 and "DONE" in p.stderr, p.stderr
        written = out.read_bytes()
        mine = bammodel.bgzf_decompress(written)
        assert mine[:recs[0]["off"]] == data[:recs[0]["off"]] and written.endswith(EOF)
        got.append(mine[recs[0]["off"]:])
        left = (tmp_path / name / "chromosome.bam.bai").read_bytes()
        assert left == bm.bai_model(written)
        bamindex.index_bam(gpu_ctx, str(out), str(tmp_path / name / "again.bai"), n_threads=2)
        assert (tmp_path / name / "again.bai").read_bytes() == left
        assert sorted(os.listdir(tmp_path / name)) == ["again.bai", "chromosome.bam", "chromosome.bam.bai"]
    placed = b"".join(data[r["off"]:r["off"] + r["length"]] for r in recs if r["ref_id"] >= 0)
    assert b"".join(got) == placed and all(got) and len(placed) < len(data) - recs[0]["off"]
