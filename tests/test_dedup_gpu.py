"""DeduplicateMolecule on the GPU against tests/dedupmodel.py, output bytes and every counter: the hand-built files in one segment and in
segments that cut their records, the scan and wave edges of the record count, the reader's state across 64-line boundaries, the molecule
table's probe loop, wrap-around and key comparison, one molecule over three segments, the writer's copy lengths, the errors of DESIGN.md
section 8f's deviation list, `bin/java`, ComputeConsensus's output fed in twice, and a seeded run of about 50,000 records."""
import importlib
import os
import random
import subprocess

import pytest

import bammodel
import consensusmodel as cm
import dedupmodel as dm
import tagbammodel as tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("lines", "records", "null_records", "skipped_lines", "molecules", "bytes_written")


@pytest.fixture(scope="module")
def dd(pkg):
    return importlib.import_module("sicelore_amd.dedupmolecule")


@pytest.fixture(scope="module")
def lib(pkg):
    return importlib.import_module("sicelore_amd.lib")


def run(dd, ctx, tmp_path, data, name="in.fq", select=True, **kw):
    """file to file, compared with the model -> (info, output bytes)"""
    src, dst = tmp_path / name, tmp_path / ("out_" + name)
    src.write_bytes(data)
    info = dd.deduplicate_molecule(ctx, str(src), str(dst), select=select, **kw)
    want, cnt = dm.dedup(data, fasta=not name.endswith(".fq"), select=select)
    got = dst.read_bytes()
    assert got == want
    assert {k: info[k] for k in COUNTERS} == cnt
    assert info["segments"] == len(info["reads"])
    return info, got


def fastq(recs):
    """recs: (ids0, ids1, rn, seq[, qual])"""
    return b"".join(b"@%s-%s-%d\n%s\n+\n%s\n" % (r[0], r[1], r[2], r[3], r[4] if len(r) > 4 else b"I" * len(r[3])) for r in recs)


def some_records(n, n_keys=None):
    n_keys = n_keys or max(1, n - n // 3)
    return [(b"BC%d" % (i * 7 % n_keys), b"U%d" % (i * 7 % n_keys % 5), i * 11 % 4 + 1, b"ACGT"[i % 4:i % 4 + 1] * (i * 5 % 9 + 1)) for i in range(n)]


def cut_records(data, reads, fasta=False):
    """the records that the end of a read of the file falls into: their lines come from different reads"""
    ends = [at + n for at, n, _used in reads[:-1]]
    return [r for r in dm.read_records(data, fasta)[0] if any(r["start"] < e < r["end"] for e in ends)]


HAND = [(dm.HAND_FASTQ, "in.fq", True), (dm.HAND_FASTQ, "in.fq", False), (dm.HAND_FASTA, "in.fa", True)]


@pytest.mark.parametrize("data,name,select", HAND, ids=["fastq_select", "fastq_first", "fasta"])
def test_hand_built_one_segment(dd, gpu_ctx, tmp_path, data, name, select):
    info, _ = run(dd, gpu_ctx, tmp_path, data, name, select)
    assert info["segments"] == 1


@pytest.mark.parametrize("data,name,select", HAND, ids=["fastq_select", "fastq_first", "fasta"])
def test_hand_built_segments_cut_the_records(dd, gpu_ctx, tmp_path, data, name, select):
    info, _ = run(dd, gpu_ctx, tmp_path, data, name, select, segment_bytes=40 if name == "in.fq" else 17)
    assert info["segments"] >= 4
    assert cut_records(data, info["reads"], name == "in.fa")
    assert sum(used < n for _at, n, used in info["reads"]) >= 4               # what a read's end cut was read again


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_record_counts(dd, gpu_ctx, tmp_path, n):
    run(dd, gpu_ctx, tmp_path, fastq(some_records(n)))


@pytest.mark.parametrize("data", [b"", b"nothing here\n\n+\nthat starts a record"], ids=["empty", "junk"])
def test_no_record_at_all(dd, gpu_ctx, tmp_path, data):
    info, got = run(dd, gpu_ctx, tmp_path, data)
    assert got == b"" and (tmp_path / "out_in.fq").exists()
    assert (info["records"], info["molecules"], info["null_records"], info["bytes_written"]) == (0, 0, 0, 0)
    assert info["lines"] == info["skipped_lines"] == (4 if data else 0)


def test_reader_state_across_64_line_boundaries(dd, gpu_ctx, tmp_path):
    tail = fastq(some_records(5))
    markers = b"".join(b"@k%d-u-1\n" % i for i in range(70))                 # 17 records of four '@' lines, then two that take the next two lines
    info, _ = run(dd, gpu_ctx, tmp_path, markers + b"AC\n+\nII\n" + tail)
    assert (info["records"], info["skipped_lines"]) == (18 + 5, 1)
    junk = b"".join(b"junk %d\n" % i for i in range(130))
    info, _ = run(dd, gpu_ctx, tmp_path, tail + junk + tail + junk[:77] + b"\n" + tail)
    assert (info["records"], info["skipped_lines"]) == (15, 130 + 10 + 1)
    fa = b"".join(b">k%d-u-1\n" % i for i in range(71)) + b"x\n>z-u-1\nAC\n"
    info, _ = run(dd, gpu_ctx, tmp_path, fa, "in.fa")
    assert (info["records"], info["skipped_lines"]) == (36 + 1, 0)


def test_table_one_chain(dd, gpu_ctx, tmp_path):
    recs = [(b"K%d" % i, b"u", 1, b"AC") for i in range(200)]
    info, _ = run(dd, gpu_ctx, tmp_path, fastq(recs), hash_bits=0)
    assert info["table_slots"] == 512 and info["molecules"] == 200
    assert info["probe_steps"] == 199 * 200 // 2 and info["wraps"] == 0       # the key that ends in slot j passed j slots, whatever the order


@pytest.mark.parametrize("n,slots", [(65, 256), (64, 128)])
def test_table_wraps_past_the_end(dd, gpu_ctx, tmp_path, n, slots):
    """keys chosen with the model's FNV-1a: three whose home is the last slot, so two of them find it taken and go on at slot 0.  (Two
    slots per record or more: 65 records get 256 slots, 128 slots are what 64 records get.)"""
    home = lambda i: dm.fnv1a(b"K%du" % i) & (slots - 1)                      # noqa: E731
    last = [i for i in range(20000) if home(i) == slots - 1][:3]
    rest = [i for i in range(20000) if home(i) != slots - 1][:n - 3]
    assert len(last) == 3
    order = rest[:10] + last[:1] + rest[10:] + last[1:]
    recs = [(b"K%d" % i, b"u", 1, b"AC") for i in order]
    assert sum(dm.fnv1a(r["key"]) & (slots - 1) == slots - 1 for r in dm.read_records(fastq(recs))[0]) == 3
    info, _ = run(dd, gpu_ctx, tmp_path, fastq(recs))
    assert info["table_slots"] == slots and info["molecules"] == n
    assert info["wraps"] >= 2


def test_table_keys_that_are_prefixes(dd, gpu_ctx, tmp_path):
    names = [b"A-B", b"AB-C", b"AB-D", b"A-", b"-", b"ABC-D", b"AB-", b"-AB", b"AC-B", b"ABD-", b"A-BC"]
    recs = [tuple(n.split(b"-")) + (i % 3 + 1, b"ACGT"[:i % 4 + 1]) for i, n in enumerate(names * 3)]
    keys = {a + b for a, b in (n.split(b"-") for n in names)}
    assert keys == {b"AB", b"ABC", b"ABD", b"A", b"", b"ABCD", b"ACB"}
    for bits in (0, 64):                                                      # one chain: every key is compared with every other
        info, _ = run(dd, gpu_ctx, tmp_path, fastq(recs), hash_bits=bits)
        assert info["molecules"] == len(keys)


def test_one_molecule_over_three_segments(dd, gpu_ctx, tmp_path):
    special = {100: (9, b"C" * 20), 300: (8, b"G" * 50), 500: (9, b"T" * 50), 700: (9, b"A" * 50), 900: (9, b"C" * 20), 950: (8, b"G" * 50)}
    recs = [(b"CELL", b"UMI", *special.get(i, (5, b"ACGTACGTAC"))) for i in range(1001)]
    data = fastq(recs)
    info, got = run(dd, gpu_ctx, tmp_path, data, segment_bytes=len(data) // 3 + 200)
    assert got == fastq([recs[500]]) and info["segments"] == 3
    winner = dm.read_records(data)[0][500]
    at, _n, used = info["reads"][1]
    assert at <= winner["start"] and winner["end"] <= at + used
    info, got = run(dd, gpu_ctx, tmp_path, data, select=False, segment_bytes=len(data) // 3 + 200)
    assert got == fastq([recs[0]])


def test_writer_lengths(dd, gpu_ctx, tmp_path):
    rng = random.Random(5)
    seq = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))               # noqa: E731
    recs = []
    for k, n in enumerate([0, 1, 63, 64, 65, 5000, 2, 3, 4, 5, 6, 7] + [100] * 40):
        recs.append((b"B" * (k % 5), b"U%d" % k, 7 if k % 2 else 2147483647, seq(n), seq(n + (k % 3) - (1 if n else 0))))
    recs.insert(3, (recs[0][0], recs[0][1], 1, b"ACGT"))                       # a record that loses, between winners
    data = fastq(recs)
    run(dd, gpu_ctx, tmp_path, data)
    info, _ = run(dd, gpu_ctx, tmp_path, data, segment_bytes=2600)
    assert info["segments"] >= 3
    held = set(dm.fold(dm.read_records(data)[0]).values())
    per_read = [[i for i, r in enumerate(dm.read_records(data)[0]) if at <= r["start"] and r["end"] <= at + used] for at, _n, used in info["reads"]]
    assert any(len(p) >= 2 and p[0] in held and p[-1] in held for p in per_read)   # winners first and last in their segment's output


@pytest.mark.parametrize("segment_bytes", [256 << 20, 12])
@pytest.mark.parametrize("name", sorted(dm.ERROR_CASES))
def test_errors_name_the_line(dd, lib, gpu_ctx, tmp_path, name, segment_bytes):
    data, fasta, line = dm.ERROR_CASES[name]
    src, dst = tmp_path / ("in.fa" if fasta else "in.fq"), tmp_path / "out"
    src.write_bytes(data)
    for select in (True, False):
        with pytest.raises(lib.DedupError, match=f"line {line}:") as e:
            dd.deduplicate_molecule(gpu_ctx, str(src), str(dst), select=select, segment_bytes=segment_bytes)
        assert e.value.line == line and not dst.exists()


def test_library_status_and_call_order(lib, gpu_ctx):
    import numpy as np
    h = lib.Dedup(gpu_ctx)
    with pytest.raises(lib.SmiError, match="last segment has not been added"):
        h.select()
    assert h.add_segment(np.frombuffer(b"@a-b-1\nAC\n+\nII\n@c-d", dtype=np.uint8), False) == 15
    with pytest.raises(lib.DedupError) as e:
        h.add_segment(np.frombuffer(b"@c-d\nAC\n+\nII\n", dtype=np.uint8), True)
    assert e.value.line == 5
    with pytest.raises(lib.SmiError, match="already closed"):
        h.add_segment(np.frombuffer(b"@c-d-1\nAC\n+\nII\n", dtype=np.uint8), True)
    h.close()
    with pytest.raises(lib.SmiError, match="hash_bits"):
        lib.Dedup(gpu_ctx, hash_bits=65)


def test_gz_refused_by_name(dd, lib, gpu_ctx, tmp_path):
    (tmp_path / "m.fastq.gz").write_bytes(b"\x1f\x8b")
    with pytest.raises(lib.SmiError, match=".gz input is not read"):
        dd.deduplicate_molecule(gpu_ctx, str(tmp_path / "m.fastq.gz"), str(tmp_path / "out.fq"))
    assert not (tmp_path / "out.fq").exists()


def test_bin_java_child_process(pkg, gpu_ctx, tmp_path):
    (tmp_path / "in.fq").write_bytes(dm.HAND_FASTQ)
    java = os.path.join(ROOT, "sicelore-2.1_amd", "bin", "java")
    r = subprocess.run(["bash", java, "-jar", "Jar/Sicelore-2.1.jar", "DeduplicateMolecule", "-I", str(tmp_path / "in.fq"), "-O", str(tmp_path / "out.fq"),
                        "-SELECT", "true", "-VALIDATION_STRINGENCY", "SILENT"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.fq").read_bytes() == dm.dedup(dm.HAND_FASTQ)[0]
    log = r.stderr.split("\n")
    for line in ("loadFastQ\tSTART...", "loadFastQ\t21 sequences loaded", "loadFastQ tso\t0", "loadFastQ\t16 molecules", "writeFastQ\tSTART...",
                 "writeFastQ\tEND..."):
        assert line in log
    assert log.index("loadFastQ\t21 sequences loaded") < log.index("loadFastQ\t16 molecules") < log.index("writeFastQ\tSTART...")


def test_consensus_output_fed_in_twice(dd, gpu_ctx, tmp_path):
    """what ComputeConsensus writes per chromosome, concatenated: the second copy has a larger rn for some molecules, which then win"""
    head, refs = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:100000\n", [("chr1", 100000)]
    mols = [("AAAA-1", "CCCC", ["ACGTACGTAA"]), ("AAAA-1", "GGGG", ["TTTTACGT", "TTTTACGTAC"]), ("CCCC-1", "CCCC", ["GATTACA"]),
            ("GGGG-1", "TTTT", ["ACACACAC", "ACACACACAC"])]
    records = [bammodel.bam_record(f"r{k}_{j}", 0, 0, 10, 60, [("M", 4)], "ACGT",
                                   aux=tm.aux_z("BC", bc) + tm.aux_z("U8", umi) + tm.aux_z("IG", "gene") + tm.aux_z("US", s))
               for k, (bc, umi, reads) in enumerate(mols) for j, s in enumerate(reads)]
    fq, cnt = cm.compute_consensus(bammodel.bam_bytes(head, refs, records))
    first = dm.read_records(fq)[0]
    assert cnt["molecules"] == len(first) == 4
    raised = {first[1]["key"], first[3]["key"]}
    second = b"".join(dm.render(dict(r, rn=r["rn"] + 3, seq=r["seq"][:-1], qual=r["qual"][:-1]) if r["key"] in raised else r) for r in first)
    info, got = run(dd, gpu_ctx, tmp_path, fq + second)
    out = dm.read_records(got)[0]
    assert sorted(r["key"] for r in out) == sorted(r["key"] for r in first) and info["molecules"] == 4
    for r in out:
        src = next(x for x in first if x["key"] == r["key"])
        assert (r["rn"], r["seq"]) == ((src["rn"] + 3, src["seq"][:-1]) if r["key"] in raised else (src["rn"], src["seq"]))


def test_seeded_50000_records_six_segments(dd, gpu_ctx, tmp_path):
    rng = random.Random(20211)
    keys = [(bytes(rng.choices(b"ACGT", k=16)), bytes(rng.choices(b"ACGT", k=12))) for _ in range(40000)]
    recs = []
    for i in range(50000):
        bc, umi = keys[i] if i < 40000 else keys[int(rng.random() ** 3 * 40000)]
        n = rng.randrange(0, 120)
        recs.append((bc, umi, rng.randrange(1, 12), bytes(rng.choices(b"ACGT", k=n)), bytes(rng.choices(range(33, 74), k=n))))
    rng.shuffle(recs)
    data = fastq(recs)
    sizes = list(dm.group_sizes(data).values())
    classes = [sum(s == 1 for s in sizes), sum(s == 2 for s in sizes), sum(s >= 3 for s in sizes)]
    assert all(classes) and len(sizes) == 40000
    info, _ = run(dd, gpu_ctx, tmp_path, data, segment_bytes=len(data) // 6 + 600)
    assert info["segments"] == 6 and info["molecules"] == 40000
