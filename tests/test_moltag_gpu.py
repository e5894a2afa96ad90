"""`AddBamMoleculeTags` and `AddGeneNameTag` on the device (K-NAME, K-GENE, K-EDIT: smi_moltag.hip) against tests/moltagmodel.py: the output
BAM (inflated) byte for byte, every counter, the read a stopped run names, and main.nf:217 / :235 / :252 through bin/java."""
import gzip
import importlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import bammodel
import moltagcases as mc
import moltagmodel as mm
import tagbammodel as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("records", "tagged", "total_reads", "wrong_strand", "right_strand", "ambiguous_fixed", "ambiguous_rejected", "multi_gene_records", "with_gene",
            "genes")


@pytest.fixture(scope="module")
def mt(pkg):
    return importlib.import_module("sicelore_amd.moltags")


@pytest.fixture(scope="module")
def lib(pkg):
    return importlib.import_module("sicelore_amd.lib")


def _write(tmp_path, bam, block=0xFF00):
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bam, block=block))
    return str(tmp_path / "in.bam"), str(tmp_path / "out.bam")


def _molecule(mt, ctx, tmp_path, records, block=0xFF00, segment_bytes=256 << 20, **tags):
    bam = mc.bam_of([("chr1", 10 ** 6)], records)
    src, dst = _write(tmp_path, bam, block)
    info = mt.add_bam_molecule_tags(ctx, src, dst, segment_bytes=segment_bytes, **tags)
    want, cnt = mm.add_molecule_tags(bam, tags.get("cell_tag", "BC"), tags.get("umi_tag", "U8"), tags.get("rn_tag", "RN"))
    raw = open(dst, "rb").read()
    assert raw.endswith(mt.BGZF_EOF) and bammodel.bgzf_decompress(raw) == want
    assert {k: info[k] for k in cnt} == cnt
    return info


def _gene(mt, ctx, tmp_path, refflat, refs, records, block=0xFF00, segment_bytes=256 << 20, model=None, **opt):
    bam = mc.bam_of(refs, records)
    src, dst = _write(tmp_path, bam, block)
    (tmp_path / "g.refFlat").write_text(refflat)
    log = io.StringIO()
    info = mt.add_gene_name_tag(ctx, src, dst, str(tmp_path / "g.refFlat"), segment_bytes=segment_bytes, log=log, **opt)
    want, cnt, dec = mm.add_gene_name_tag(bam, refflat, opt.get("gene_tag", "GE"), opt.get("strand_tag", "GS"), opt.get("function_tag", "XF"),
                                          opt.get("use_strand_info", True), opt.get("allow_multi_gene_reads", True), model=model)
    got = bammodel.bgzf_decompress(open(dst, "rb").read())
    if got != want:                                   # name the first record that differs
        a, b = bammodel.parse_bam(got)[2], bammodel.parse_bam(want)[2]
        bad = [(x["name"], x["aux"], y["aux"]) for x, y in zip(a, b) if x != y][:3]
        raise AssertionError(f"{len(a)} / {len(b)} records, first differences: {bad}")
    assert {k: info[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS}
    assert log.getvalue().splitlines() == [f"Loaded {cnt['genes']} transcripts.", mt.METRICS.format(**cnt)]
    return info, cnt, dec


# ---- AddBamMoleculeTags ------------------------------------------------------------------------------------------------------------------
def test_names_and_attributes_match_the_model(mt, gpu_ctx, tmp_path):
    info = _molecule(mt, gpu_ctx, tmp_path, mc.name_records())
    assert info["tagged"] == sum(bool(mm.name_edits(n)) for n in mc.NAMES) >= 20


def test_names_in_small_segments(mt, gpu_ctx, tmp_path):
    _molecule(mt, gpu_ctx, tmp_path, mc.name_records() * 3, block=700, segment_bytes=900)


def test_option_tags_may_coincide(mt, gpu_ctx, tmp_path):
    _molecule(mt, gpu_ctx, tmp_path, mc.name_records(), cell_tag="XX", umi_tag="XX", rn_tag="RN")
    _molecule(mt, gpu_ctx, tmp_path, mc.name_records(), cell_tag="XX", umi_tag="YY", rn_tag="XX")
    _molecule(mt, gpu_ctx, tmp_path, mc.name_records(), cell_tag="U9", umi_tag="AA", rn_tag="NM")


def test_attribute_limit(mt, lib, gpu_ctx, tmp_path):
    fits = [mc.rec("A-B-3", [("M", 4)], aux=mc.many_attrs(61)), mc.rec("plain", [("M", 4)], aux=mc.many_attrs(64)),
            mc.rec("A-B-3", [("M", 4)], aux=mc.many_attrs(61) + tm.aux_z("BC", "x") + tm.aux_z("U8", "x") + tm.aux_z("RN", "x"))]
    _molecule(mt, gpu_ctx, tmp_path, fits)
    src, dst = _write(tmp_path, mc.bam_of([("chr1", 10 ** 6)], fits + [mc.rec("A-B-3", [("M", 4)], aux=mc.many_attrs(62))]))
    os.remove(dst)
    with pytest.raises(lib.SmiError, match="more than 64 attributes"):
        mt.add_bam_molecule_tags(gpu_ctx, src, dst)
    assert os.listdir(tmp_path) == ["in.bam"]
    for bad, msg in ((tm.aux_h("XH", "abc"), "H attribute that is not hex"), (b"XXZnonul", "malformed or unknown attribute type")):
        src, dst = _write(tmp_path, mc.bam_of([("chr1", 10 ** 6)], [mc.rec("plain", [("M", 4)], aux=bad)]))
        with pytest.raises(lib.SmiError, match=msg):
            mt.add_bam_molecule_tags(gpu_ctx, src, dst)
    for record in mc.damaged_records().values():                    # every way an attribute list goes wrong: SMI_TAG_BAD_AUX
        src, dst = _write(tmp_path, mc.bam_of([("chr1", 10 ** 6)], mc.name_records() + [record]))
        with pytest.raises(lib.SmiError, match="malformed or unknown attribute type"):
            mt.add_bam_molecule_tags(gpu_ctx, src, dst)


@pytest.mark.parametrize("stop", mc.STOP_NAMES)
@pytest.mark.parametrize("segmented", [False, True])
def test_a_third_piece_that_is_no_int_stops_the_run(mt, lib, gpu_ctx, tmp_path, stop, segmented):
    records = mc.name_records() * 2 + [mc.rec(stop, [("M", 8)])] + mc.name_records() + [mc.rec("A-B-x", [("M", 8)])]
    bam = mc.bam_of([("chr1", 10 ** 6)], records)
    with pytest.raises(mm.Stop) as want:
        mm.add_molecule_tags(bam)
    assert want.value.read == stop
    src, dst = _write(tmp_path, bam, block=700 if segmented else 0xFF00)
    with pytest.raises(lib.MolTagError) as e:
        mt.add_bam_molecule_tags(gpu_ctx, src, dst, segment_bytes=900 if segmented else 256 << 20)
    assert (e.value.read, e.value.record) == (stop, want.value.record) and stop in str(e.value)
    assert os.listdir(tmp_path) == ["in.bam"]                     # no output file, no temporary file
    cli = importlib.import_module("sicelore_amd.cli")
    if not segmented:
        assert cli.main(["AddBamMoleculeTags", "-I", src, "-O", dst]) == 1 and not os.path.exists(dst)


# ---- AddGeneNameTag ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(mc.GENE_CASES))
def test_gene_cases_match_the_model(mt, gpu_ctx, tmp_path, case):
    refflat, refs, records = mc.GENE_CASES[case]()
    info, cnt, dec = _gene(mt, gpu_ctx, tmp_path, refflat, refs, records)
    if case == "search":
        kept = {r: len(d["genes"]) for r, d in zip([x["name"] for x in bammodel.parse_bam(mc.bam_of(refs, records))[2]], dec) if d}
        assert kept["under0"] == 0 and kept["under1"] == 1 and kept["under200"] == 100 and kept["under65r"] == 32 and kept["widefar"] == 1
    if case in ("search", "strand", "collision"):               # the host's ordering path is taken, and only for these records
        assert 0 < info["multi_gene_records"] <= info["records"] and info["multi_gene_records"] == cnt["multi_gene_records"]


@pytest.mark.parametrize("case", ["strand", "search", "collision"])
@pytest.mark.parametrize("opt", [dict(use_strand_info=False), dict(allow_multi_gene_reads=False), dict(use_strand_info=False, allow_multi_gene_reads=False),
                                 dict(gene_tag="XG", strand_tag="XG", function_tag="XG"), dict(function_tag="GE")])
def test_gene_options(mt, gpu_ctx, tmp_path, case, opt):
    refflat, refs, records = mc.GENE_CASES[case]()
    info, cnt, _ = _gene(mt, gpu_ctx, tmp_path, refflat, refs, records, **opt)
    if not opt.get("allow_multi_gene_reads", True):
        assert info["with_gene"] == 0 and info["multi_gene_records"] == 0
    if not opt.get("use_strand_info", True):
        assert info["total_reads"] == 0 and info["right_strand"] == 0


def test_gene_cases_in_small_segments(mt, gpu_ctx, tmp_path):
    refflat, refs, records = mc.strand_case()
    _gene(mt, gpu_ctx, tmp_path, refflat, refs, records * 20, block=900, segment_bytes=1200)


@pytest.mark.parametrize("segmented", [False, True])
def test_a_record_without_a_block_under_a_gene_stops_the_run(mt, lib, gpu_ctx, tmp_path, segmented):
    refflat, refs, records = mc.error_case(True)
    records = mc.strand_case()[2] * 8 + records
    src, dst = _write(tmp_path, mc.bam_of(refs, records), block=900 if segmented else 0xFF00)
    (tmp_path / "g.refFlat").write_text(refflat)
    with pytest.raises(lib.MolTagError) as e:
        mt.add_gene_name_tag(gpu_ctx, src, dst, str(tmp_path / "g.refFlat"), segment_bytes=1200 if segmented else 256 << 20)
    assert (e.value.read, e.value.record) == ("clipped", 89)
    assert sorted(os.listdir(tmp_path)) == ["g.refFlat", "in.bam"]
    refflat, refs, records = mc.error_case(False)                 # under no gene: XF INTERGENIC
    _gene(mt, gpu_ctx, tmp_path, refflat, refs, records)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
# sicelore-nf/main.nf:217, :235 and :252, verbatim
STEP217 = "$params.java -jar $params.javaXmx $params.sicelore AddBamMoleculeTags -I $bam -O molecules.tags.bam -CELLTAG $params.CELLTAG -UMITAG $params.UMITAG -RNTAG $params.RNTAG"
STEP235 = ("$params.java -jar $params.javaXmx $params.sicelore AddGeneNameTag -I $bam -O molecules.tags.GE.bam -REFFLAT $params.refflat -GENETAG $params.GENETAG "
           "-ALLOW_MULTI_GENE_READS $params.ALLOW_MULTI_GENE_READS -USE_STRAND_INFO $params.USE_STRAND_INFO -VALIDATION_STRINGENCY SILENT")
STEP252 = ("$params.java -jar $params.javaXmx $params.sicelore IsoformMatrix -I $bam -REFFLAT $params.refflat -CSV $csv -OUTDIR ./ -PREFIX $params.PREFIX "
           "-CELLTAG $params.CELLTAG -UMITAG $params.UMITAG -GENETAG $params.GENETAG -TSOENDTAG $params.TSOENDTAG -POLYASTARTTAG $params.POLYASTARTTAG "
           "-CDNATAG $params.CDNATAG -USTAG $params.USTAG -RNTAG $params.RNTAG -MAPQV0 $params.MAPQV0 -DELTA $params.DELTA -METHOD $params.METHOD "
           "-ISOBAM $params.ISOBAM -AMBIGUOUS_ASSIGN $params.AMBIGUOUS_ASSIGN -VALIDATION_STRINGENCY SILENT")
PARAMS = {"$params.javaXmx": "-Xmx4G", "$params.sicelore": "Jar/Sicelore-2.1.jar", "$params.CELLTAG": "BC", "$params.UMITAG": "U8", "$params.RNTAG": "RN",
          "$params.GENETAG": "GE", "$params.ALLOW_MULTI_GENE_READS": "true", "$params.USE_STRAND_INFO": "true", "$params.refflat": "genes.refFlat",
          "$params.PREFIX": "sicelore", "$params.TSOENDTAG": "TE", "$params.POLYASTARTTAG": "PS", "$params.CDNATAG": "CS", "$params.USTAG": "US",
          "$params.MAPQV0": "false", "$params.DELTA": "2", "$params.METHOD": "STRICT", "$params.ISOBAM": "false", "$params.AMBIGUOUS_ASSIGN": "false"}


def _nf(cmd):
    for k in sorted(PARAMS, key=len, reverse=True):
        cmd = cmd.replace(k, PARAMS[k])
    return cmd.replace("$params.java", "$java")


def test_main_nf_217_235_252_through_bin_java(pkg, tmp_path):
    """molecule names as DeduplicateMolecule writes them (BC-UMI-rn) at spliced loci -> :217 -> :235 -> :252 as child processes; both BAMs equal
    the model's and IsoformMatrix counts the molecules the model says carry a gene"""
    import isoformmodel as im

    ref = "".join(f"GENE{g}\tTX{g}\tchr12\t{'+-'[g & 1]}\t{19_000 + 4_000 * g}\t{22_500 + 4_000 * g}\t{19_100 + 4_000 * g}\t{22_400 + 4_000 * g}\t2\t"
                  f"{19_000 + 4_000 * g},{20_999 + 4_000 * g},\t{20_100 + 4_000 * g},{22_500 + 4_000 * g},\n" for g in range(8))
    rng = np.random.default_rng(5)
    rows = []
    for m in range(400):
        g = m % 10                                                   # loci 8 and 9 lie under no gene
        a, b = 20_100 + 4_000 * g, 21_000 + 4_000 * g
        strand = 16 if (g & 1) ^ (m % 7 == 0) else 0                  # one in seven on the wrong strand
        rows.append((a - 80, f"CELL{m % 12:04d}ACGTACGTAC-UMI{m:09d}-{1 + int(rng.integers(9))}", strand,
                     [("S", 10), ("M", 81), ("N", b - a - 1), ("M", 70), ("S", 5)]))
    rows.sort()
    recs = [bammodel.bam_record(nm, fl, 0, p0, 30, cig, "C" * sum(n for o, n in cig if o in "MS")) for p0, nm, fl, cig in rows]
    bam = bammodel.bam_bytes("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr12\tLN:100000000\n", [("chr12", 10 ** 8)], recs)
    (tmp_path / "molecules.bam").write_bytes(bammodel.bgzf_compress(bam, block=16384))
    (tmp_path / "genes.refFlat").write_text(ref)
    (tmp_path / "barcodes.csv").write_text("".join(f"CELL{c:04d}ACGTACGTAC\n" for c in range(0, 12, 2)))
    java = "bash " + os.path.join(ROOT, "sicelore-2.1_amd", "bin", "java")
    env = dict(os.environ, PYTHON=sys.executable, java=java, csv="barcodes.csv")
    want1, cnt1 = mm.add_molecule_tags(bam)
    want2, cnt2, _ = mm.add_gene_name_tag(want1, ref)
    for step, src, dst, want in ((STEP217, "molecules.bam", "molecules.tags.bam", want1), (STEP235, "molecules.tags.bam", "molecules.tags.GE.bam", want2)):
        r = subprocess.run(["bash", "-c", _nf(step)], env=dict(env, bam=src), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert bammodel.bgzf_decompress((tmp_path / dst).read_bytes()) == want
    assert "Loaded 8 transcripts." in r.stderr and mt_metrics(cnt2) in r.stderr and r.stdout == ""
    assert cnt1["tagged"] == 400 and 0 < cnt2["with_gene"] < 320 and cnt2["wrong_strand"] > 0
    r = subprocess.run(["bash", "-c", _nf(STEP252)], env=dict(env, bam="molecules.tags.GE.bam"), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    _outs, cnt = im.isoform_matrix(want2, ref, (tmp_path / "barcodes.csv").read_text())
    log = dict(ln.split(",", 1) for ln in (tmp_path / "sicelore.log").read_text().splitlines() if "," in ln)
    assert int(log["Total molecules"]) == cnt["molecules"] and int(log["SAMrecords no gene"]) == cnt["no_gene"] == 400 - cnt2["with_gene"]


def mt_metrics(c):
    return (f"TOTAL READS [{c['total_reads']}] CORRECT_STRAND [{c['right_strand']}]  WRONG_STRAND [{c['wrong_strand']}] "
            f"AMBIGUOUS_STRAND_FIXED [{c['ambiguous_fixed']}] AMBIGUOUS REJECTED READS [{c['ambiguous_rejected']}]")


# ---- seeded ----------------------------------------------------------------------------------------------------------------------------
def test_seeded_run_over_chr12_in_six_segments(mt, gpu_ctx, tmp_path):
    """about 50 k spliced records over the refFlat head (what they reach is counted in DESIGN.md section 8g)"""
    refflat = gzip.open(os.path.join(ROOT, "tests", "golden", "chr12_head1500.refFlat.gz"), "rt").read()
    rows = [ln.split("\t") for ln in refflat.split("\n") if ln and not ln.startswith("#")]
    rng = np.random.default_rng(11)
    records = []
    for m in range(50_000):
        f = rows[int(rng.integers(len(rows)))]
        es, ee = [int(x) for x in f[9].split(",") if x], [int(x) for x in f[10].split(",") if x]
        k = int(rng.integers(len(es)))
        mode = int(rng.integers(10))
        if mode == 0:                                                # somewhere around the transcript
            pos, cig = max(1, int(f[4]) - 500 + int(rng.integers(int(f[5]) - int(f[4]) + 1000))), [("M", int(rng.integers(20, 120)))]
        else:                                                        # from exon k over up to three junctions, ends jittered
            pos = max(1, es[k] + 1 + int(rng.integers(-8, max(1, ee[k] - es[k]))))
            cig, at = [("S", int(rng.integers(0, 30)))], pos
            for j in range(k, min(len(es), k + 1 + int(rng.integers(4)))):
                end = ee[j] + (int(rng.integers(-3, 4)) if rng.integers(4) == 0 else 0)
                if end < at:
                    break
                cig.append(("M", end - at + 1))
                if j + 1 < len(es) and es[j + 1] + 1 > end + 1:
                    cig.append(("N", es[j + 1] + 1 - end - 1))
                    at = es[j + 1] + 1
            if cig[-1][0] == "N":
                cig.pop()
            if len(cig) == 1:
                cig.append(("M", 30))
            cig = [c for c in cig if c[1] > 0]
        flag = 16 if (f[3] == "-") ^ (rng.integers(8) == 0) else 0
        if rng.integers(200) == 0:
            flag |= 4
        records.append(mc.rec(f"C{int(rng.integers(500)):04d}-U{m:08d}-{int(rng.integers(1, 40))}", cig, pos, 0, flag))
    refs = [("chr12", 133275309)]
    bam = mc.bam_of(refs, records)
    seg = len(bammodel.bgzf_compress(bam)) // 6 + 1
    info, cnt, dec = _gene(mt, gpu_ctx, tmp_path, refflat, refs, records, segment_bytes=seg)
    assert cnt["with_gene"] > 30_000 and cnt["multi_gene_records"] > 100 and cnt["wrong_strand"] > 1000 and cnt["ambiguous_fixed"] > 0
    assert cnt["tagged"] < cnt["records"] == 50_000
    _molecule(mt, gpu_ctx, tmp_path, records, segment_bytes=seg)
