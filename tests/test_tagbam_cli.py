"""`tagbamwithread` without a GPU: the model of tests/tagbammodel.py against hand-worked cases, and the command line's argument errors
(commons-cli's messages, exit code 1), which end the run before any device is touched."""
import os
import struct
import subprocess
import sys

import bammodel
import tagbammodel as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = bammodel.bam_bytes("@HD\tVN:1.6\tSO:coordinate\n", [("chr1", 1000), ("chr2", 1000)], [])


def _rec(name, flag=0, ref=0, aux=b"", seq="ACGT"):
    return bammodel.bam_record(name, flag, ref, 10, 60, [("M", len(seq))], seq, aux=aux)


def _records(out):
    _, _, recs = bammodel.parse_bam(out)
    return recs


def test_fastq_key_is_cut_at_the_first_space_and_the_last_record_wins():
    fq = tm.fastq_text([("a x y", "AC", "II"), ("b\tc d", "GG", "##"), (" lead", "T", "5"), ("a z", "TTT", "!!!"), ("e", "", "")])
    m = tm.fastq_map(fq)
    assert m == {b"a": (b"TTT", b"!!!"), b"b\tc": (b"GG", b"##"), b"": (b"T", b"5"), b"e": (b"", b"")}
    assert tm.fastq_map(fq.replace(b"\n", b"\r\n")) == m


def test_records_are_dropped_reported_or_tagged():
    fq = tm.fastq_text([("r1 comment", "ACGTA", "ABCDE"), ("r2", "GG", "FF")])
    recs = [_rec("r1"), _rec("r1", flag=4, ref=-1), _rec("r1", flag=4, ref=1), _rec("gone"), _rec("r2", flag=256), _rec("r2", flag=2048)]
    out, miss, counts = tm.tag_bam(fq, HEAD + b"".join(recs), "US")
    assert counts == dict(records=6, written=4, unmapped=1, missing=1)
    assert miss == ["ERROR: Did not find read for  SAM record, name: gone Check whether fastq and BAM file correspond !"]
    got = _records(out)
    assert [(r["name"], r["flag"], r["ref_id"]) for r in got] == [("r1", 0, 0), ("r1", 4, 1), ("r2", 256, 0), ("r2", 2048, 0)]
    assert got[0]["aux"] == b"USZACGTA\0" and got[2]["aux"] == b"USZGG\0"
    assert out.startswith(HEAD)


def test_attributes_are_rewritten_as_htsjdk_writes_them():
    fq = tm.fastq_text([("r", "ACG", "III")])
    aux = (tm.aux_z("US", "old") + tm.aux_int("NM", "i", 3) + tm.aux_int("XI", "I", 70000) + tm.aux_int("XS", "s", -200)
           + tm.aux_h("XH", "0aFF") + tm.aux_z("AA", "keep") + tm.aux_int("NM", "C", 250))
    out, _, _ = tm.tag_bam(fq, HEAD + _rec("r", aux=aux), "US", "QS")
    a = _records(out)[0]["aux"]
    # ordered by binary tag (second char << 8 | first): AA 0x4141, XH 0x4858, XI 0x4958, NM 0x4d4e, QS 0x5351, US 0x5355, XS 0x5358
    want = (tm.aux_z("AA", "keep") + b"XHBc" + struct.pack("<I", 2) + b"\x0a\xff" + tm.aux_int("XI", "i", 70000) + tm.aux_int("NM", "C", 250)
            + tm.aux_z("QS", "III") + tm.aux_z("US", "ACG") + tm.aux_int("XS", "s", -200))
    assert a == want


def _cli(args, cwd, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, "sicelore-2.1_amd")] + args, cwd=cwd, capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, **(env or {})))


def test_cli_argument_errors(tmp_path):
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(HEAD))
    (tmp_path / "r.fastq").write_bytes(tm.fastq_text([("r", "A", "I")]))
    ok = ["--inFastq", "r.fastq", "--inBam", "in.bam", "--outBam", "o.bam"]
    for args, needle in (
            (["--inBam", "a.bam"], "Missing required options: f, o, r"),
            (["-o", "x.bam", "-r", "US"], "Missing required options: b, f"),
            (ok + ["--readTag", "U"], "read tag must be two characters"),
            (ok + ["--readTag", "USX"], "read tag must be two characters"),
            (ok + ["--readTag", "US", "--qvTag", "Q"], "QV tag must be two characters"),
            (ok + ["--readTag", "US", "--frobnicate", "1"], "Command line parsing error"),
            (ok + ["--readTag"], "Command line parsing error"),
            (["--inFastq", "none.fastq", "--inBam", "in.bam", "--outBam", "o.bam", "--readTag", "US"], "none.fastq"),
            (["--inFastq", "r.fastq", "--inBam", "none.bam", "--outBam", "o.bam", "--readTag", "US"], "none.bam")):
        r = _cli(["tagbamwithread"] + args, str(tmp_path))
        assert r.returncode == 1 and needle in r.stderr, (args, r.returncode, r.stderr[-400:])
    assert not (tmp_path / "o.bam").exists()
    r = _cli(["tagbamwithread"] + ok + ["--readTag", "US"], str(tmp_path), env={"WORLD_SIZE": "2"})
    assert r.returncode == 1 and "one process" in r.stderr
    r = _cli(["mergestats"], str(tmp_path))
    assert r.returncode == 1 and "sub-command" in r.stderr and "mergestats" in r.stderr
