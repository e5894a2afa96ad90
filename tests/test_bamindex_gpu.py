"""BamIndex on the GPU (K-BAI, smi_bamindex.hip, through bamindex.index_bam): every case of tests/baicases.py in one segment and again in
four or more, the product's bytes against the model's (tests/baimodel.py) and the cover property of the specification's reader on the
product's file; the stops, through the function and through bamindex.py's main; the index as a by-product of the four BAM writers; and the
consumer, assignumis over two shards, on the product's index.  tests/test_bamindex_cpu.py asserts that each input holds the edges named
here."""
import importlib
import io
import os

import numpy as np
import pytest

import __graft_entry__ as graft
import baicases as bc
import baimodel as bm
import bammodel

pytestmark = pytest.mark.gpu
ONE = 256 << 20


def _mod(name):
    return importlib.import_module(f"{graft.PKG_NAME}.{name}")


@pytest.fixture(scope="module")
def bi(pkg):
    return _mod("bamindex")


@pytest.fixture(scope="module")
def lib(pkg):
    return _mod("lib")


def _index(bi, ctx, tmp_path, raw, segment_bytes, name="in.bam"):
    p = tmp_path / name
    p.write_bytes(raw)
    info = bi.index_bam(ctx, str(p), segment_bytes=segment_bytes, n_threads=2)
    data = (tmp_path / f"{name}.bai").read_bytes()
    assert info["bytes_written"] == len(data) and not [f for f in os.listdir(tmp_path) if ".tmp" in f]
    return data, info


def _both(bi, ctx, tmp_path, raw, seg):
    """the index of one segment and of the segmented run: both equal the model's -> (index, info of the segmented run)"""
    want = bm.bai_model(raw)
    one, info1 = _index(bi, ctx, tmp_path, raw, ONE)
    many, info = _index(bi, ctx, tmp_path, raw, seg)
    assert one == want and many == want
    assert info1["segments"] <= 1 and info["records"] == info1["records"]
    return many, info


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def test_hand_built_file(bi, gpu_ctx, tmp_path):
    raw, seg = bc.hand()
    bai, info = _both(bi, gpu_ctx, tmp_path, raw, seg)
    assert (info["records"], info["refs_with_records"], info["chunks"], info["no_coor"], info["segments"]) == (3, 1, 2, 1, 2)
    assert bm.uncovered(raw, bai) == []
    assert set(info["stage_ms"]) == {"record", "order", "chunk", "linear", "finish"} and info["seconds"]["device"] > 0


def test_extents_and_bins(bi, gpu_ctx, tmp_path):
    """CIGARs of 0 .. 65,535 operations over all nine kinds, lengths of 0, a placed flag 0x4, a CG placeholder, records on both sides of
    and exactly on the borders of every bin level, end = 2^29, pos = 2^29 - 1, an N of 2^27 bases (8,193 windows)"""
    raw, seg = bc.extents()
    bai, info = _both(bi, gpu_ctx, tmp_path, raw, seg)
    assert info["segments"] >= 4 and info["windows"] == 1 << 15
    assert bm.uncovered(raw, bai, bc.random_regions([("big", 1 << 29)], 200, seed=3)) == []


@pytest.mark.parametrize("name", ["offsets", "offsets_border"])
def test_offsets(bi, gpu_ctx, tmp_path, name):
    """records from a block's first byte to its last, over three blocks, an empty block in mid-file (offsets_border: right behind the
    first segment's last record), no EOF block, records cut by the segment borders"""
    raw, seg = bc.CASES[name]()
    bai, info = _both(bi, gpu_ctx, tmp_path, raw, seg)
    assert info["segments"] >= 4 and info["blocks"] == sum(1 for b in bm.bgzf_walk(raw) if b[2])
    assert bm.uncovered(raw, bai) == []


def test_chunks(bi, gpu_ctx, tmp_path):
    """runs of 1, 2, 63, 64 and 65 records, bins A B A B over 130 records, a run over two segment borders, bin 0 with a chunk from the
    first and one from the last segment"""
    raw, seg = bc.chunks()
    bai, info = _both(bi, gpu_ctx, tmp_path, raw, seg)
    assert info["segments"] >= 4 and info["chunks"] == 1 + 5 + 130 + 1 + 1
    assert bm.uncovered(raw, bai) == []


@pytest.mark.parametrize("name", ["no_references", "only_unplaced", "many_references"])
def test_references(bi, gpu_ctx, tmp_path, name):
    raw, seg = bc.CASES[name]()
    bai, info = _both(bi, gpu_ctx, tmp_path, raw, seg)
    want = dict(no_references=(0, 0, 0, 0), only_unplaced=(40, 0, 0, 40), many_references=(2000, 1000, 2000, 0))[name]
    assert (info["records"], info["refs_with_records"], info["chunks"], info["no_coor"]) == want
    assert bm.uncovered(raw, bai) == []


def test_linear_index(bi, gpu_ctx, tmp_path):
    """leading empty windows, a gap of 10 windows, the record of 8,193 windows"""
    raw, seg = bc.linear()
    bai, info = _both(bi, gpu_ctx, tmp_path, raw, seg)
    assert info["segments"] >= 4
    assert bm.uncovered(raw, bai, bc.random_regions([("chr1", 1 << 29)], 200, seed=5)) == []


# ---- the stops ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bc.stops()))
@pytest.mark.parametrize("segmented", [False, True])
def test_stops_name_the_read_and_leave_no_file(bi, lib, gpu_ctx, tmp_path, capsys, monkeypatch, name, segmented):
    raw, seg, record, read, kind = bc.stops()[name]
    p = tmp_path / "in.bam"
    p.write_bytes(raw)
    with pytest.raises(lib.BamIndexError) as e:
        bi.index_bam(gpu_ctx, str(p), segment_bytes=seg if segmented else ONE, n_threads=2)
    assert (e.value.record, e.value.read) == (record, read)
    assert read in str(e.value) and f"record {record}" in str(e.value)
    assert ("BAI cannot hold the position" in str(e.value)) == (kind == "far")
    assert os.listdir(tmp_path) == ["in.bam"]
    # through the command line: exit code 1, the same names on stderr, still nothing written
    monkeypatch.setattr(_mod("cli"), "_context", lambda: gpu_ctx)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    if segmented:
        real = bi.index_bam
        monkeypatch.setattr(bi, "index_bam", lambda ctx, a, b=None, **kw: real(ctx, a, b, segment_bytes=seg, **kw))
    assert bi.main([str(p)]) == 1
    err = capsys.readouterr().err
    assert f"read {read} (record {record})" in err and "was not written" in err
    assert os.listdir(tmp_path) == ["in.bam"]


# ---- a seeded case -------------------------------------------------------------------------------------------------------------------------
def test_seeded_20k_records_in_segments_twice(bi, gpu_ctx, tmp_path):
    raw = bc.seeded()
    want = bm.bai_model(raw)
    a, info_a = _index(bi, gpu_ctx, tmp_path, raw, 100_000)
    b, info_b = _index(bi, gpu_ctx, tmp_path, raw, 30_000)
    assert a == b and a == want
    assert info_a["records"] == 20300 and info_a["no_coor"] == 300 and info_a["refs_with_records"] == 5
    assert 4 <= info_a["segments"] < info_b["segments"]
    assert bm.uncovered(raw, a, bc.random_regions(bm.records_of(raw)[0], 200)) == []


# ---- the writers ---------------------------------------------------------------------------------------------------------------------------
def _writer(which, ctx, tmp_path, src, dst, index, **kw):
    """one of the four BAM writers from src to dst -> its info"""
    if which == "molecule":
        return _mod("moltags").add_bam_molecule_tags(ctx, src, dst, segment_bytes=1500, n_threads=2, index=index, **kw)
    if which == "gene":
        rf = tmp_path / "genes.refFlat"
        rf.write_text(bc.WRITER_REFFLAT)
        return _mod("moltags").add_gene_name_tag(ctx, src, dst, str(rf), segment_bytes=1500, n_threads=2, index=index, **kw)
    if which == "read":
        return _mod("fusionprep").add_bam_read_tags(ctx, src, dst, segment_bytes=1500, n_threads=2, index=index, **kw)
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(bc.writer_fastq())
    return _mod("tagbamwithread").tag_bam_with_reads(ctx, str(fq), src, dst, "US", "QS", segment_bytes=1500, n_threads=2, index=index,
                                                    err=io.StringIO(), **kw)


def _bai_of(which, dst):
    return dst[:-4] + ".bai" if which == "tagbam" else dst + ".bai"


@pytest.mark.parametrize("which", ["molecule", "gene", "read", "tagbam"])
def test_writers_leave_the_index_of_what_they_wrote(bi, gpu_ctx, tmp_path, which):
    _refs, raw = bc.writer_input()
    src = tmp_path / "in.bam"
    src.write_bytes(raw)
    plain, dst = str(tmp_path / "plain.bam"), str(tmp_path / "out.bam")
    info0 = _writer(which, gpu_ctx, tmp_path, str(src), plain, False)
    assert "index" not in info0 and not [f for f in os.listdir(tmp_path) if f.endswith(".bai")]       # the default: as before
    info = _writer(which, gpu_ctx, tmp_path, str(src), dst, True)
    written = open(dst, "rb").read()
    assert written == open(plain, "rb").read()
    got = open(_bai_of(which, dst), "rb").read()
    assert info["index_error"] is None and info["index"]["bytes_written"] == len(got) and info["index"]["path"] == _bai_of(which, dst)
    assert got == bm.bai_model(written)
    again, info2 = _index(bi, gpu_ctx, tmp_path, written, ONE, name="again.bam")
    assert got == again
    n = 600 if which == "tagbam" else 605                                     # tagbamwithread drops the records without a reference
    assert info["index"]["records"] == info2["records"] == n and info["index"]["segments"] >= 4
    assert bm.uncovered(written, got) == []
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]


@pytest.mark.parametrize("which", ["molecule", "tagbam"])
def test_writers_keep_the_bam_of_an_unsorted_input(gpu_ctx, tmp_path, which):
    _refs, raw = bc.writer_input(unsorted=True)
    src = tmp_path / "in.bam"
    src.write_bytes(raw)
    plain, dst = str(tmp_path / "plain.bam"), str(tmp_path / "out.bam")
    _writer(which, gpu_ctx, tmp_path, str(src), plain, False)
    info = _writer(which, gpu_ctx, tmp_path, str(src), dst, True)
    assert info["index"] is None and "record 201" in info["index_error"] and "out of coordinate order" in info["index_error"]
    assert "was not written" in info["index_error"] and "the BAM is complete" in info["index_error"]
    assert open(dst, "rb").read() == open(plain, "rb").read()
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".bai") or ".tmp" in f]


# ---- the consumer --------------------------------------------------------------------------------------------------------------------------
def _three_chromosomes(pkg, synth, ctx, tmp_path):
    """the three-chromosome BAM of tests/test_assignumis_shards_gpu.py's construction (names from a real pass 2, four unmapped records last),
    its refFlat, and the index bammodel.bai_bytes gives it"""
    scanfastq = _mod("scanfastq")
    rng = np.random.default_rng(71)
    wl = synth.make_whitelist(40_000, seed=7101)
    used = synth.pick_used(wl, 6, seed=7102)
    n_mol, copies = 90, 4
    mol = synth.gen_reads(n_mol, used, seed=7103, err=0.0, q_mean=20.0)
    seqs, quals, mol_of = [], [], []
    for m in range(n_mol):
        s, q = synth.materialize(mol, m)
        for _ in range(copies):
            t = list(s)
            for p in rng.integers(0, len(t), max(1, len(t) // 50)):
                t[p] = "ACGT"[rng.integers(0, 4)]
            seqs.append("".join(t))
            quals.append(q)
            mol_of.append(m)
    ctx.set_barcode_set(used.numpy().astype(np.uint64), mode=0)
    text = "".join(f"@read{i} runid=x\n{s}\n+\n{q}\n" for i, (s, q) in enumerate(zip(seqs, quals))).encode()
    rows = []
    for r in scanfastq.ReadScanner(ctx, max_ed=1, split_chimeras=False).pass2_chunk(text):
        qname = r["name"].split(" ")[0]
        if "_FAILED" in qname:
            continue
        m = mol_of[r["source"]]
        rows.append((m % 3, 30_000 + 4_000 * (m // 3 % 12) + int(rng.integers(0, 80)), qname, 16 if m & 1 else 0, r["length"]))
    rows.sort()
    tail = [(-1, -1, f"unmapped{k}", 4, 300) for k in range(4)]
    block = 4096
    header = bammodel.bam_bytes("@HD\tVN:1.6\tSO:coordinate\n", [("chr1", 10 ** 6), ("chr2", 10 ** 6), ("chr3", 10 ** 6)], [])
    brecs = [bammodel.bam_record(nm, fl, ref, p0, 30, [("M", L)] if ref >= 0 else [], "C" * L) for ref, p0, nm, fl, L in rows + tail]
    data = header + b"".join(brecs)
    offs = bammodel.bgzf_block_offsets(data, block)
    at, idx = len(header), []
    for (ref, p0, _nm, _fl, L), b in zip(rows + tail, brecs):
        idx.append((ref, p0, p0 + L, bammodel.virtual_offset(at, block, offs), bammodel.virtual_offset(at + len(b), block, offs) or ((offs[-1] + 1) << 16)))
        at += len(b)
    in_bam = str(tmp_path / "in.bam")
    with open(in_bam, "wb") as f:
        f.write(bammodel.bgzf_compress(data, block=block))
    refflat = ""
    for c in range(3):
        for g in range(12):
            a = 29_500 + 4_000 * g
            refflat += f"G{c}_{g}\tT{c}_{g}\tchr{c + 1}\t+\t{a}\t{a + 3000}\t{a}\t{a + 3000}\t1\t{a},\t{a + 3000},\n"
    return in_bam, refflat, bammodel.bai_bytes(3, idx, meta=True), len(rows) + len(tail)


def test_the_products_index_drives_assignumis_over_two_shards(pkg, synth, bi, gpu_ctx, tmp_path):
    au = _mod("assignumis")
    in_bam, refflat, model_bai, n_records = _three_chromosomes(pkg, synth, gpu_ctx, tmp_path)
    info = bi.index_bam(gpu_ctx, in_bam, segment_bytes=9_000, n_threads=2)
    assert info["records"] == n_records and info["no_coor"] == 4 and info["refs_with_records"] == 3
    assert open(in_bam + ".bai", "rb").read() == bm.bai_model(open(in_bam, "rb").read())
    ext = au.bai_ref_extents(in_bam + ".bai")
    assert ext == au.bai_ref_extents_bytes(model_bai) and None not in ext
    for world in (1, 2, 3, 4):
        assert au.plan_shards(ext, world) == au.plan_shards(au.bai_ref_extents_bytes(model_bai), world)
    one, many = str(tmp_path / "one"), str(tmp_path / "many")
    a = au.assignumis_stream(gpu_ctx, in_bam, one, segment_bytes=9_000, chunk_size=90, n_threads=2, refflat=refflat)
    infos = [au.assignumis_stream(gpu_ctx, in_bam, many, segment_bytes=9_000, chunk_size=90, n_threads=2, refflat=refflat, shard=(r, 2)) for r in range(2)]
    assert sum(i["records"] for i in infos) == a["records"] == n_records and all(i["records"] > 0 for i in infos)
    m = au.merge_shards(many, 2)
    assert m["gene_keys_order_dependent"] == 0
    for name in (".bam", "_umifound_.bam"):
        assert bammodel.bgzf_decompress(open(many + name, "rb").read()) == bammodel.bgzf_decompress(open(one + name, "rb").read()), name
    for name in (".genecounts.tsv", ".UMIdepths.tsv"):
        assert open(many + name).read() == open(one + name).read(), name
