"""`tagbamwithread` on the device (K-TAG, smi_tagbam.hip) against the model of tests/tagbammodel.py: the output BAM (inflated) byte for
byte and the stderr miss lines, line for line."""
import gzip
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import bammodel
import tagbammodel as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_TEXT = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:100000\n@SQ\tSN:chr2\tLN:100000\n"
REFS = [("chr1", 100000), ("chr2", 100000)]


@pytest.fixture(scope="module")
def tb(pkg):
    import importlib

    return importlib.import_module("sicelore_amd.tagbamwithread")


@pytest.fixture(scope="module")
def lib(pkg):
    import importlib

    return importlib.import_module("sicelore_amd.lib")


def _rec(name, flag=0, ref=0, pos=10, aux=b"", seq="ACGTACGT"):
    return bammodel.bam_record(name, flag, ref, pos, 60, [("M", len(seq))], seq, aux=aux)


def _check(tb, ctx, tmp_path, fastq, records, read_tag="US", qv_tag=None, gz=False, block=0xFF00, **kw):
    bam = bammodel.bam_bytes(HEAD_TEXT, REFS, records)
    fq_path = tmp_path / ("in.fastq.gz" if gz else "in.fastq")
    fq_path.write_bytes(gzip.compress(fastq) if gz else fastq)
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bam, block=block))
    err = io.StringIO()
    info = tb.tag_bam_with_reads(ctx, str(fq_path), str(tmp_path / "in.bam"), str(tmp_path / "out.bam"), read_tag, qv_tag, err=err, **kw)
    want, miss, counts = tm.tag_bam(fastq, bam, read_tag, qv_tag)
    raw = open(tmp_path / "out.bam", "rb").read()
    assert raw.endswith(tb.BGZF_EOF)
    got = bammodel.bgzf_decompress(raw)
    assert got == want
    assert err.getvalue().splitlines() == miss
    assert {k: info[k] for k in counts} == counts
    return info


def _mixed_case():
    fastq = tm.fastq_text([("r1 runid=abc ch=12", "ACGTTGCA", "ABCDEFGH"), ("r2\ttabbed comment", "GGGG", "####"), (" leading", "T", "5"),
                           ("dup first", "AAAA", "1111"), ("r3", "CCCCC", "IIIII"), ("dup second", "CCCCCC", "222222"),
                           ("r5", "ACGTACGTAC" * 30, "#" * 300)])
    records = [
        _rec("r1"),
        _rec("r1", flag=4, ref=-1, pos=-1),                                          # no reference: dropped
        _rec("r1", flag=4, ref=1, pos=50),                                           # flag 4 with a position: kept
        _rec("r2\ttabbed"),
        _rec(""),                                                                    # the key of the header with a leading space
        _rec("dup", flag=256), _rec("dup", flag=2048), _rec("dup"),
        _rec("missing_one"),
        _rec("r3", aux=tm.aux_z("US", "stale") + tm.aux_int("NM", "i", 2) + tm.aux_z("QS", "oldq")),
        _rec("r3", flag=16, aux=tm.aux_int("XI", "I", 70000) + tm.aux_int("XS", "s", -200) + tm.aux_h("XH", "0aFF") + tm.aux_a("XA", "Q")
             + tm.aux_f("XF", 1.5) + tm.aux_b("XB", "s", [1, -2, 3]) + tm.aux_z("AA", "keep") + tm.aux_int("XI", "C", 250) + tm.aux_h("XE", "")),
        _rec("r5", aux=tm.aux_int("a1", "S", 65535) + tm.aux_int("a2", "i", -70000) + tm.aux_int("a3", "I", 2 ** 32 - 1)),
        _rec("missing_two", ref=1),
        _rec("r2", flag=4, ref=-1),
    ]
    return fastq, records


@pytest.mark.parametrize("qv", [None, "QS"])
@pytest.mark.parametrize("hash_bits", [0, 4])
def test_mixed_records_match_the_model(tb, gpu_ctx, tmp_path, qv, hash_bits):
    fastq, records = _mixed_case()
    info = _check(tb, gpu_ctx, tmp_path, fastq, records, qv_tag=qv, hash_bits=hash_bits, gz=qv is None)
    assert info["missing"] == 2 and info["unmapped"] == 2


def test_zlib_writer_and_other_tags(tb, gpu_ctx, tmp_path):
    fastq, records = _mixed_case()
    _check(tb, gpu_ctx, tmp_path, fastq, records, read_tag="XR", qv_tag="XQ", bgzf="zlib", n_threads=3)


def _many(n, seed):
    rng = np.random.default_rng(seed)
    names = [f"read_{i:06d}_{rng.integers(0, 1 << 30):x}" for i in range(n)]
    rows = []
    for i, nm in enumerate(names):
        L = int(rng.integers(1, 400))
        seq = "".join(rng.choice(list("ACGTN"), L))
        qual = "".join(chr(33 + int(q)) for q in rng.integers(0, 60, L))
        rows.append((nm + (f" comment={i}" if i % 3 else ""), seq, qual))
    for i in rng.choice(n, n // 20, replace=False):             # re-reads of some names later in the file: the last one wins
        seq = "ACGT" * int(rng.integers(1, 5))
        rows.append((names[int(i)] + " again", seq, "I" * len(seq)))
    recs = []
    for j in range(n + n // 10):
        nm = names[int(rng.integers(0, n))] if j < n else f"absent_{j}"
        ref = -1 if j % 97 == 0 else int(rng.integers(0, 2))
        aux = tm.aux_int("NM", "i", int(rng.integers(0, 300))) + (tm.aux_z("US", "x") if j % 5 == 0 else b"")
        recs.append(_rec(nm, flag=[0, 16, 256, 2048][j % 4], ref=ref, pos=j, aux=aux, seq="ACGT"[: 1 + j % 4]))
    return tm.fastq_text(rows), recs


def test_every_probe_collides_on_20k_records(tb, gpu_ctx, tmp_path):
    """hash_bits=4: sixteen hash values for 20 k names -- every insert and every probe walks the byte compare"""
    fastq, recs = _many(20_000, 11)
    info = _check(tb, gpu_ctx, tmp_path, fastq, recs, qv_tag="QS", hash_bits=4)
    assert info["written"] > 18_000 and info["missing"] == 2_000 - sum(1 for j in range(20_000, 22_000) if j % 97 == 0)


def test_segments_cut_records(tb, gpu_ctx, tmp_path):
    """small BGZF blocks and a segment of a few blocks: records and the header itself are cut across segments"""
    fastq, recs = _many(3_000, 12)
    info = _check(tb, gpu_ctx, tmp_path, fastq, recs, qv_tag="QS", block=700, segment_bytes=1500)
    assert info["records"] == len(recs)


def test_empty_fastq_and_header_only_bam(tb, gpu_ctx, tmp_path):
    _, records = _mixed_case()
    info = _check(tb, gpu_ctx, tmp_path, b"", records)
    assert info["written"] == 0 and info["fastq_records"] == 0
    info = _check(tb, gpu_ctx, tmp_path, tm.fastq_text([("r1", "A", "I")]), [], qv_tag="QS")
    assert info["records"] == 0


def test_malformed_fastq_is_an_error(pkg, gpu_ctx):
    from sicelore_amd import lib

    for text in (b"@r\nAC\n+\nI\n", b"r\nA\n+\nI\n", b"@r\nA\n+\nI\n@s\nA\n"):
        with pytest.raises(lib.SmiError, match="malformed"):
            lib.TagBam(gpu_ctx, text, "US", "QS")
    with pytest.raises(lib.SmiError, match="read tag"):
        lib.TagBam(gpu_ctx, b"", "U")


def test_segment_size_only_call_then_write(pkg, gpu_ctx):
    """out smaller than the records: the sized segment stays on the device and the next call writes it"""
    from sicelore_amd import lib

    fastq, records = _mixed_case()
    bam = np.frombuffer(bammodel.bam_bytes(HEAD_TEXT, REFS, records), dtype=np.uint8).copy()
    _t, _r, start = lib.bam_header(bam)
    recs, _end = lib.bam_index_records(bam, start, cap=64)
    t = lib.TagBam(gpu_ctx, fastq, "US", "QS")
    out, missing, unmapped = t.segment(bam, recs, out=np.zeros(16, dtype=np.uint8))
    want, miss, _c = tm.tag_bam(fastq, bam.tobytes(), "US", "QS")
    assert bam[:start].tobytes() + out.tobytes() == want and len(missing) == len(miss) and unmapped == 2
    assert set(t.stage_ms()) == {"key", "build", "probe", "size", "assemble"}
    t.close()


# ---- K-TAG-ASM through lib.TagBam.segment: what the rewrite shared with K-EDIT (smi_auxedit.h) must keep ----------------------------------
FASTQ_AB = tm.fastq_text([("a", "ACGT", "IIII"), ("b", "GG", "##")])


def _attrs(n, first=0):
    """n distinct one-byte integer attributes (lower-case tags: none is US or QS)"""
    return b"".join(tm.aux_int("%c%c" % (ord("a") + k // 26, ord("a") + k % 26), "C", k % 200) for k in range(first, first + n))


def _segment(lib, ctx, records, qv="QS", fastq=FASTQ_AB):
    """records through one TagBam.segment -> (what the model writes for them, the records written, missing, unmapped, stage ms)"""
    bam = np.frombuffer(bammodel.bam_bytes(HEAD_TEXT, REFS, records), dtype=np.uint8).copy()
    _t, _r, start = lib.bam_header(bam)
    recs, _end = lib.bam_index_records(bam, start, cap=len(records) + 1)
    assert len(recs) == len(records)
    t = lib.TagBam(ctx, fastq, "US", qv)
    try:
        out, missing, unmapped = t.segment(bam, recs)
        want = tm.tag_bam(fastq, bam.tobytes(), "US", qv)[0][start:]      # (behind the call: the model has no limit and no error of its own)
        return want, out.tobytes(), list(missing), unmapped, t.stage_ms()
    finally:
        t.close()


@pytest.mark.parametrize("qv, n_in", [("QS", 62), (None, 63)])
def test_attribute_limit_is_reached_with_the_new_tags(lib, gpu_ctx, qv, n_in):
    """64 attributes are written, the 65th is the error -- counted after US (and QS) are added"""
    plain = _rec("b", aux=tm.aux_int("NM", "i", 2))
    want, got, _m, _u, _ms = _segment(lib, gpu_ctx, [plain, _rec("a", aux=_attrs(n_in)), plain], qv)
    assert got == want
    with pytest.raises(lib.SmiError, match="smi_tagbam_segment: a record's attributes cannot be rewritten: more than 64 attributes;"):
        _segment(lib, gpu_ctx, [plain, _rec("a", aux=_attrs(n_in + 1)), plain], qv)


def test_attribute_limit_counts_a_tag_once(lib, gpu_ctx):
    """stale US / QS among 64 inputs are replaced, not added; a tag repeated in the input counts once"""
    stale = _attrs(31) + tm.aux_z("US", "stale") + _attrs(31, first=31) + tm.aux_z("QS", "old")
    repeated = _attrs(62) + _attrs(62) + tm.aux_int("aa", "i", -70000)       # 125 fields, 62 tags
    want, got, _m, _u, _ms = _segment(lib, gpu_ctx, [_rec("a", aux=stale), _rec("b", aux=repeated)])
    assert got == want
    with pytest.raises(lib.SmiError, match="more than 64 attributes"):
        _segment(lib, gpu_ctx, [_rec("b", aux=_attrs(63) + _attrs(63))])


@pytest.mark.parametrize("aux", [_attrs(70), tm.aux_h("XH", "abc")], ids=["70_attributes", "odd_hex"])
def test_a_dropped_record_is_never_parsed(lib, gpu_ctx, aux):
    """a record without a reference and one whose name the FASTQ lacks are dropped before their attributes are looked at: attributes that
    would be an error in a written record are none here"""
    good = _rec("a", aux=tm.aux_z("US", "stale") + tm.aux_int("NM", "i", 2))
    records = [good, _rec("a", flag=4, ref=-1, pos=-1, aux=aux), _rec("b"), _rec("absent", aux=aux), good]
    want, got, missing, unmapped, _ms = _segment(lib, gpu_ctx, records)
    assert got == want and missing == [3] and unmapped == 1
    assert len(bammodel.parse_bam(bammodel.bam_bytes(HEAD_TEXT, REFS, []) + got)[2]) == 3
    with pytest.raises(lib.SmiError, match="cannot be rewritten"):            # the same attributes on a record that is written
        _segment(lib, gpu_ctx, [good, _rec("b", aux=aux)])


def test_all_records_dropped_and_empty_segment(lib, gpu_ctx):
    """nothing to write: total 0 and no WRITE launch (its stage time stays 0); n == 0 through the two-call protocol"""
    want, got, missing, unmapped, ms = _segment(lib, gpu_ctx, [_rec("a", flag=4, ref=-1, pos=-1), _rec("absent"), _rec("b", ref=-1)])
    assert want == b"" and got == b"" and missing == [1] and unmapped == 2 and ms["assemble"] == 0.0 and ms["size"] > 0.0
    want, got, missing, unmapped, ms = _segment(lib, gpu_ctx, [])
    assert want == b"" and got == b"" and missing == [] and unmapped == 0 and ms["assemble"] == 0.0
    import ctypes

    t = lib.TagBam(gpu_ctx, FASTQ_AB, "US", "QS")
    try:
        n_out, n_miss, n_unm = ctypes.c_size_t(7), ctypes.c_int32(7), ctypes.c_int32(7)
        buf = np.zeros(16, dtype=np.uint8)
        for out, cap in ((None, 0), (buf.ctypes.data, buf.size)):              # sizes first, then the same arguments with a buffer
            assert t._lib.smi_tagbam_segment(t._h, None, 0, None, 0, out, cap, ctypes.byref(n_out), None, ctypes.byref(n_miss), ctypes.byref(n_unm)) == 0
            assert (n_out.value, n_miss.value, n_unm.value) == (0, 0, 0)
        assert t.stage_ms()["assemble"] == 0.0
    finally:
        t.close()


# sicelore-nf/main.nf:116, verbatim
STEP4 = "$params.java -jar $params.javaXmx $params.nanopore tagbamwithread --inFastq $fastqgz --inBam $bam --outBam parsedbamseq.bam --readTag US --qvTag QS"


def test_main_nf_step4_on_what_scanfastq_wrote(pkg, synth, gpu_ctx, tmp_path):
    """synth reads -> run_files.run -> the passed *.fastq.gz concatenated (main.nf:33) -> a BAM of alignments for a subset of those names ->
    the main.nf:116 command line through bin/java: the names scanfastq writes are the keys the join finds"""
    import importlib

    import torch

    run_files = importlib.import_module("sicelore_amd.run_files")
    dev = torch.device("cuda", 0)
    wl = synth.make_whitelist(30_000, seed=5401, device=dev)
    used = synth.pick_used(wl, 40, seed=5402)
    fastqdir, scandir = tmp_path / "fastq", tmp_path / "scan"
    run_files.write_synthetic_dir(synth, str(fastqdir), 2, 1200, used, dev, seed=5410, chimera_frac=0.05)
    run_files.run(gpu_ctx, str(fastqdir), str(scandir), max_ed=1, n_workers=4, reads_per_chunk=1000, whitelist_keys=np.sort(wl.cpu().numpy().astype(np.uint64)),
                  compress=True)
    passed = sorted((scandir / "passed").iterdir())
    assert passed and all(p.name.endswith("_passed.fastq.gz") for p in passed)
    fastqgz = tmp_path / "fastq_pass.fastq.gz"
    with open(fastqgz, "wb") as f:                    # `pigz -dc | pigz`: one stream of the concatenated texts (here: their members)
        for p in passed:
            f.write(p.read_bytes())
    text = gzip.open(fastqgz).read()
    names = [ln[1:].split(b" ")[0].decode() for ln in text.split(b"\n")[0::4] if ln]
    assert len(names) > 1000
    rng = np.random.default_rng(7)
    pick = sorted(rng.choice(len(names), len(names) // 2, replace=False))
    recs = [_rec(names[int(i)], flag=16 if k % 3 == 0 else 0, pos=100 + k) for k, i in enumerate(pick)] + [_rec("not_a_read", pos=99_000)]
    bam = bammodel.bam_bytes(HEAD_TEXT, REFS, recs)
    (tmp_path / "passedParsed.bam").write_bytes(bammodel.bgzf_compress(bam, block=16384))
    os.environ["PYTHON"] = sys.executable
    java = "bash " + os.path.join(ROOT, "sicelore-2.1_amd", "bin", "java")
    cmd = STEP4.replace("$params.javaXmx", "-Xmx4G").replace("$params.nanopore", "Jar/NanoporeBC_UMI_finder-2.1.jar")
    cmd = cmd.replace("$params.java", "$java")
    env = dict(os.environ, java=java, fastqgz=str(fastqgz), bam=str(tmp_path / "passedParsed.bam"))
    r = subprocess.run(["bash", "-c", cmd], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want, miss, counts = tm.tag_bam(text, bam, "US", "QS")
    assert counts["written"] == len(pick) and miss == [tm.MISS.format("not_a_read")]
    assert bammodel.bgzf_decompress(open(tmp_path / "parsedbamseq.bam", "rb").read()) == want
    assert [ln for ln in r.stderr.splitlines() if ln.startswith("ERROR: Did not find")] == miss
