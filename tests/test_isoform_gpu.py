"""IsoformMatrix on the GPU against tests/isoformmodel.py, every output file byte for byte and every counter: the STRICT cases on a
hand-built BAM, a seeded run of about 50 k molecules on the chr12 refFlat, the HBM spill path of K-ISO and the multi-block render of K-MTX."""
import gzip
import importlib
import os

import numpy as np
import pytest

import bammodel
import isoformmodel as im
import tagbammodel as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "@HD\tVN:1.6\n@SQ\tSN:chr12\tLN:2000000\n"
REFS = [("chr12", 2000000)]


@pytest.fixture(scope="module")
def iso(pkg):
    return importlib.import_module("sicelore_amd.isoformmatrix")


def _rec(name, cigar, pos0, bc, umi, gene, flag=0, mapq=60, de=None, rn=None):
    aux = tm.aux_z("BC", bc) + tm.aux_z("U8", umi) + tm.aux_z("GE", gene)
    if de is not None:
        aux += tm.aux_f("de", de)
    if rn is not None:
        aux += tm.aux_int("RN", "C", rn)
    return bammodel.bam_record(name, flag, 0, pos0, mapq, cigar, "ACGT", aux=aux)


def _cigar_for(junc, pos1, jitter=0, rng=None):
    """M / N operations whose junctions are `junc` (each end moved by up to jitter) -> (pos0, cigar)"""
    cig, cur = [], pos1
    for s, e in junc:
        if rng is not None and jitter:
            s += int(rng.integers(-jitter, jitter + 1))
            e += int(rng.integers(-jitter, jitter + 1))
        cig.append(("M", max(1, s - cur + 1)))
        cur = cur + max(1, s - cur + 1)
        cig.append(("N", max(1, e - cur)))
        cur = cur + max(1, e - cur)
    cig.append(("M", 30))
    return pos1 - 1, cig


def _run(iso, ctx, tmp_path, bam, refflat, csv, **kw):
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bam, block=3000))
    (tmp_path / "r.refFlat").write_text(refflat)
    (tmp_path / "c.csv").write_text(csv)
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    info = iso.isoform_matrix(ctx, str(tmp_path / "in.bam"), str(tmp_path / "r.refFlat"), str(tmp_path / "c.csv"), str(out), prefix="t",
                              segment_bytes=9000, n_threads=3, **kw)
    mk = {k: v for k, v in kw.items() if k in ("delta", "mapqv0", "to_bulk", "isobam")}
    want, cnt = im.isoform_matrix(bam, refflat, csv, **mk)
    for name, data in want.items():
        got = (out / f"t_{name}").read_bytes()
        if name == "isobam.bam":
            assert got.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
            got = bammodel.bgzf_decompress(got)
        assert got == data, name
    assert {k: info[k] for k in cnt} == cnt
    return info, cnt


# G1: T1 (2 junctions), T1 again (PAR duplicate), T2 (other junctions); G2: one monoexon line; G3 and G4 share a region, G3 has 2 lines
REF = ("G1\tT1\tchr12\t+\t999\t3000\t999\t3000\t3\t999,1999,2999,\t1100,2100,3100,\n"
       "G1\tT1\tchr12\t+\t999\t3000\t999\t3000\t3\t999,1999,2999,\t1100,2100,3100,\n"
       "G1\tT2\tchr12\t+\t999\t3000\t999\t3000\t3\t999,1499,2999,\t1100,1600,3100,\n"
       "G1\tT3\tchr12\t+\t999\t3000\t999\t3000\t3\t999,1999,2999,\t1101,2100,3100,\n"
       "G2\tM1\tchr12\t+\t5000\t6000\t5000\t6000\t1\t5000,\t6000,\n"
       "G3\tA1\tchr12\t+\t9000\t9500\t9000\t9500\t2\t9000,9400,\t9100,9500,\n"
       "G3\tA2\tchr12\t+\t9000\t9500\t9000\t9500\t2\t9000,9300,\t9100,9500,\n"
       "G4\tB1\tchr12\t+\t9000\t9500\t9000\t9500\t2\t9000,9200,\t9100,9500,\n"
       "G5\tC1\tchr12\t+\t9000\t9500\t9000\t9500\t2\t9000,9200,\t9150,9500,\n"
       "G6\tD1\tchr12\t+\t9000\t9500\t9000\t9500\t2\t9000,9200,\t9150,9500,\n")


def _hand_records():
    t1 = [(1100, 2000), (2100, 3000)]
    R = []
    p, c = _cigar_for(t1, 1000)
    R += [_rec("onematch_a", c, p, "CELL1-1", "U1", "G1", de=0.1), _rec("onematch_b", c, p, "CELL1-1", "U1", "G1", de=0.25, rn=5)]
    p, c = _cigar_for([(1102, 2002), (2100, 3000)], 1000)                  # exactly DELTA from T1: matches
    R += [_rec("delta2", c, p, "CELL2", "U1", "G1")]
    p, c = _cigar_for([(1103, 2000), (2100, 3000)], 1000)                  # DELTA + 1 from T1, 2 from T3: T3 only
    R += [_rec("delta3", c, p, "CELL2", "U2", "G1")]
    p, c = _cigar_for([(1101, 2000), (2100, 3000)], 1000)                  # within DELTA of T1 and T3: tie, T1|G1 < T3|G1
    R += [_rec("tie", c, p, "CELL2", "U3", "G1")]
    R += [_rec("mono", [("M", 50)], 5100, "CELL1", "U2", "G2", de=1e-4)]
    p, c = _cigar_for([(9100, 9250)], 9001)                                # G3 (2 lines) vs G4 (1 line): nomatch -> G3
    R += [_rec("nomatch", c, p, "CELL3", "U1", "G4,G3")]
    R += [_rec("nomatch_tie", c, p, "CELL3", "U2", "G6,G5")]              # 1 line each: G5, the first gene of the refFlat
    R += [_rec("empty", [("M", 40)], 20000, "CELL3", "U3", "NOTAGENE")]   # no transcripts: undef / undef
    p, c = _cigar_for(t1, 1000)
    R += [_rec("notincsv", c, p, "CELLX", "U1", "G1"), _rec("ab", c, p, "CELL1", "U9", "G1,G2")]
    R += [_rec("chim", [("S", 200)] + c, p, "CELL1", "U8", "G1")]
    R += [_rec("sec0", c, p, "CELL1", "U7", "G1", flag=256, mapq=0), _rec("sec0", c, p, "CELL1", "U7", "G1", mapq=0)]
    p, c = _cigar_for([(1100, 2000)], 1000)
    R += [_rec("partial", c, p, "CELL1", "U6", "G1")]                     # one junction: no match, one junction in the set
    # the reference's CIGAR walk through the product (LongreadRecord L120-150), each record a molecule of CELL4 at T1's exons
    M, N, D, I, S, H = "M", "N", "D", "I", "S", "H"
    walks = {
        "Q1": [(M, 101), (D, 899), (M, 101), (N, 899), (M, 30)],                            # D > 20: a junction
        "Q2": [(M, 101), (D, 20), (M, 879), (N, 100), (M, 101), (N, 899), (M, 30)],         # D <= 20: none, e stays
        "Q3": [(M, 101), (D, 30), (N, 869), (M, 101), (N, 899), (M, 30)],                   # D > 20 then N: one junction twice
        "Q4": [(H, 5), (S, 3), (M, 101), (N, 899), (M, 101), (N, 899), (M, 30), (S, 4), (H, 2)],  # leading / trailing H and S
        "Q5": [(M, 50), (I, 2), (M, 51), (N, 899), (M, 101), (N, 899), (M, 30)],            # I inside an exon: a block of its own
        "Q6": [(M, 101), (N, 899), (M, 101), (N, 899)],                                     # the last operation is a gap: not looked at
        "Q7": [(M, 101), (N, 898), (M, 102), (N, 899), (M, 30)],                            # 2000 -> 1999 / 2100 -> 2101 (DELTA)
    }
    for umi, cig in walks.items():
        R += [_rec("walk_" + umi, cig, 999, "CELL4", umi, "G1", de=0.99999 if umi == "Q1" else 0.03125)]  # Q1: an E-form pctId
    R += [bammodel.bam_record("unmapped", 4, -1, -1, 0, [], "ACGT", aux=tm.aux_z("BC", "CELL4") + tm.aux_z("U8", "Q1"))]
    R += [bammodel.bam_record("nobc", 0, 0, 999, 60, [("M", 40)], "ACGT", aux=tm.aux_z("U8", "Q2") + tm.aux_z("GE", "G1"))]
    return R


@pytest.mark.parametrize("mapqv0", [False, True])
def test_hand_built_strict_cases(iso, gpu_ctx, tmp_path, mapqv0):
    bam = bammodel.bam_bytes(HEAD, REFS, _hand_records())
    info, cnt = _run(iso, gpu_ctx, tmp_path, bam, REF, "CELL1\nCELL2-1\nCELL3\nCELL4\n", mapqv0=mapqv0, to_bulk=True, isobam=True)
    assert cnt["monoexon"] >= 1 and cnt["onematch"] >= 2 and cnt["nomatch"] == 6 and cnt["chimeria"] == 1
    assert cnt["mapqv0"] == (0 if mapqv0 else 1)
    mi = (tmp_path / "out" / "t_molinfos.txt").read_bytes()
    assert b"CELL3\tU1\t1\t0\t0.0\t\tG3\tundef\n" in mi and b"E-" in mi
    jm = (tmp_path / "out" / "t_juncmatrix.txt").read_bytes()
    assert b"G1:1100-2000\t" in jm and b"G1:2100-3000\t" in jm
    # ISOBAM: every record, the raw "CELL1-1" of onematch_a keys no molecule (undef), "CELL1" of mono keys its molecule
    _t, _r, recs = bammodel.parse_bam(bammodel.bgzf_decompress((tmp_path / "out" / "t_isobam.bam").read_bytes()))
    assert len(recs) == len(_hand_records())
    by = {r["name"]: r["aux"] for r in recs}
    assert tm.aux_z("IG", "undef") in by["onematch_a"] and tm.aux_z("IG", "G2") + tm.aux_z("IT", "M1") in by["mono"]
    assert _t.startswith("@HD\tVN:1.6\tSO:unsorted\n")


def test_refflat_errors_name_the_line(pkg, gpu_ctx):
    lib = importlib.import_module("sicelore_amd.lib")
    with pytest.raises(lib.SmiError, match="REFFLAT line 2: has 3 fields"):
        lib.Isoform(gpu_ctx, REF.split("\n")[0].encode() + b"\nG1\tT1\tchr1\n", b"A\n")
    with pytest.raises(lib.SmiError, match="REFFLAT line 1: field 5 is not an integer"):
        lib.Isoform(gpu_ctx, b"G\tT\tc\t+\tx\t1\t1\t1\t1\t1,\t2,\n", b"A\n")


def test_cigar_walk_error_names_the_read(iso, gpu_ctx, tmp_path):
    bad = [bammodel.bam_record("noblock", 0, 0, 999, 60, [("S", 40)], "ACGT", aux=tm.aux_z("BC", "C") + tm.aux_z("U8", "U") + tm.aux_z("GE", "G1"))]
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bammodel.bam_bytes(HEAD, REFS, bad)))
    (tmp_path / "r.refFlat").write_text(REF)
    (tmp_path / "c.csv").write_text("C\n")
    lib = importlib.import_module("sicelore_amd.lib")
    with pytest.raises(lib.SmiError, match="read noblock: the CIGAR walk"):
        iso.isoform_matrix(gpu_ctx, str(tmp_path / "in.bam"), str(tmp_path / "r.refFlat"), str(tmp_path / "c.csv"), str(tmp_path), prefix="t")


def _chr12():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "chr12_head1500.refFlat.gz"), "rt") as f:
        return f.read()


def _seeded(n_mol, seed, jitter=3):
    rng = np.random.default_rng(seed)
    genes, by_gene, _n = im.parse_refflat(_chr12())
    multi = [g for g in genes if any(j for _t, j, _e in by_gene[g])]
    recs = []
    for m in range(n_mol):
        g = multi[int(rng.integers(len(multi)))]
        tx, junc, _ne = by_gene[g][int(rng.integers(len(by_gene[g])))]
        if not junc:
            continue
        start = max(1, junc[0][0] - 40)
        bc, umi = f"C{int(rng.integers(300)):04d}", f"U{m:07d}"
        for r in range(int(rng.integers(1, 4))):
            p, c = _cigar_for(junc, start, jitter=jitter, rng=rng)
            if any(n <= 0 for _o, n in c):
                continue
            recs.append(_rec(f"m{m}_{r}", c, p, bc, umi, g, de=float(rng.integers(0, 30)) / 100))
    csv = "".join(f"C{i:04d}-1\n" for i in range(0, 300, 2)) + "C9999\n"
    return bammodel.bam_bytes(HEAD, REFS, recs), csv


def test_seeded_50k_molecules_chr12(iso, gpu_ctx, tmp_path):
    bam, csv = _seeded(50000, 7)
    info, cnt = _run(iso, gpu_ctx, tmp_path, bam, _chr12(), csv, isobam=True)
    assert cnt["onematch"] > 10000 and cnt["ambiguous"] > 0 and cnt["nomatch"] > 0 and cnt["matrix_junctions"] > 100


def test_spill_path_and_multi_block_render(iso, gpu_ctx, tmp_path):
    bam, csv = _seeded(3000, 11)
    info, _cnt = _run(iso, gpu_ctx, tmp_path, bam, _chr12(), csv, lds_tx=2, budget_bytes=20000)
    assert info["spill"] > 100
    assert info["render_blocks"] > 10


# quickrun-2.1.sh:42 and :46, verbatim
STEP3 = "$java -jar  -Xmx4G Jar/NanoporeBC_UMI_finder-2.1.jar assignumis --inFileNanopore ${mappingdir}passed.bam -o ${umidir}passedParsed.bam --annotationFile Data/gencode.v38.chr12.refFlat"
STEP4A = "$java -jar -Xmx4g Jar/Sicelore-2.1.jar IsoformMatrix -I ${umidir}passedParsed.bam -REFFLAT Data/gencode.v38.chr12.refFlat -CSV ${siceloredir}barcodes.csv -OUTDIR $siceloredir -PREFIX reads -ISOBAM true -VALIDATION_STRINGENCY SILENT"


def test_quickrun_lines_42_and_46_through_bin_java(pkg, synth, gpu_ctx, tmp_path):
    """synthetic reads -> run_files.run (scanfastq) -> a passed.bam at eight spliced loci -> quickrun :42 (assignumis) -> :46 (IsoformMatrix,
    ISOBAM true) through bin/java: every file and the ISOBAM equal the model's on the BAM assignumis wrote"""
    import subprocess
    import sys

    import torch

    run_files = importlib.import_module("sicelore_amd.run_files")
    dev = torch.device("cuda", 0)
    wl = synth.make_whitelist(30_000, seed=6401, device=dev)
    used = synth.pick_used(wl, 40, seed=6402)
    work = tmp_path / "run"
    (work / "Data").mkdir(parents=True)
    dirs = {k: str(work / k) + "/" for k in ("fastq", "scan", "map", "umi", "sicelore")}
    for k in ("map", "umi", "sicelore"):
        os.makedirs(dirs[k])
    run_files.write_synthetic_dir(synth, dirs["fastq"], 2, 1500, used, dev, seed=6410, chimera_frac=0.05)
    run_files.run(gpu_ctx, dirs["fastq"], dirs["scan"], max_ed=1, n_workers=4, reads_per_chunk=1000,
                  whitelist_keys=np.sort(wl.cpu().numpy().astype(np.uint64)), compress=True)
    names = []
    for p in sorted(os.listdir(dirs["scan"] + "passed")):
        lines = gzip.open(dirs["scan"] + "passed/" + p).read().split(b"\n")
        names += [ln[1:].split(b" ")[0].decode() for ln in lines[0::4] if ln]
    assert len(names) > 1000
    # "mapping": two-exon alignments at eight loci, junctions jittered around the refFlat's
    rng = np.random.default_rng(6)
    rows = []
    for i, nm in enumerate(names):
        g = i % 8
        a, b = 20_100 + 4_000 * g + int(rng.integers(-3, 4)), 21_000 + 4_000 * g + int(rng.integers(-3, 4))
        p1 = a - 80
        rows.append((p1 - 1, nm, 16 if g & 1 else 0, [("S", 10), ("M", a - p1 + 1), ("N", b - a - 1), ("M", 70), ("S", 5)]))
    rows.sort()
    recs = [bammodel.bam_record(nm, fl, 0, p0, 30, cig, "C" * (sum(n for o, n in cig if o in "MS"))) for p0, nm, fl, cig in rows]
    header = bammodel.bam_bytes("@HD\tVN:1.6\tSO:coordinate\n", [("chr12", 10 ** 8)], [])
    with open(dirs["map"] + "passed.bam", "wb") as f:
        f.write(bammodel.bgzf_compress(header + b"".join(recs), block=16384))
    ref = "".join(f"GENE{g}\tTX{g}\tchr12\t+\t{19_000 + 4_000 * g}\t{22_500 + 4_000 * g}\t{19_100 + 4_000 * g}\t{22_400 + 4_000 * g}\t2\t"
                  f"{19_000 + 4_000 * g},{20_999 + 4_000 * g},\t{20_100 + 4_000 * g},{22_500 + 4_000 * g},\n" for g in range(8))
    ref += "".join(f"GENE{g}\tTX{g}b\tchr12\t+\t{19_000 + 4_000 * g}\t{22_500 + 4_000 * g}\t0\t0\t1\t{19_000 + 4_000 * g},\t{22_500 + 4_000 * g},\n"
                   for g in range(0, 8, 3))
    (work / "Data" / "gencode.v38.chr12.refFlat").write_text(ref)
    os.environ["PYTHON"] = sys.executable
    java = "bash " + os.path.join(ROOT, "sicelore-2.1_amd", "bin", "java")
    env = dict(os.environ, java=java, mappingdir=dirs["map"], umidir=dirs["umi"], siceloredir=dirs["sicelore"])
    r = subprocess.run(["bash", "-c", STEP3], env=env, cwd=str(work), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    parsed = bammodel.bgzf_decompress(open(dirs["umi"] + "passedParsed.bam", "rb").read())
    _t, _r, out = bammodel.parse_bam(parsed)
    bcs = sorted({a["aux"][a["aux"].index(b"BCZ") + 3:].split(b"\0")[0].decode() for a in out if b"BCZ" in a["aux"]})
    assert len(out) > 500 and len(bcs) > 5
    (work / "sicelore" / "barcodes.csv").write_text("".join(b + "\n" for b in bcs[::2]))   # the cell list, written here
    r = subprocess.run(["bash", "-c", STEP4A], env=env, cwd=str(work), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want, cnt = im.isoform_matrix(parsed, ref, (work / "sicelore" / "barcodes.csv").read_text(), isobam=True)
    sd = work / "sicelore"
    for name, data in want.items():
        got = (sd / f"reads_{name}").read_bytes()
        if name == "isobam.bam":
            got = bammodel.bgzf_decompress(got)
        assert got == data, name
    assert cnt["onematch"] + cnt["monoexon"] > 100
    log = (sd / "reads.log").read_text()
    assert log.startswith(f"IsoformMatrix INPUT,{dirs['umi']}passedParsed.bam\n") and f"Total molecules,{cnt['molecules']}\n" in log
