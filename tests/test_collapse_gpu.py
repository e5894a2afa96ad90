"""CollapseModel on the GPU against tests/collapsemodel.py: all five files byte for byte and every counter, on the hand-built case and the
size, threshold and order edges of tests/collapsecases.py (tests/test_collapse_cpu.py asserts that each edge is in its input)."""
import importlib
import os
import subprocess
import sys

import pytest

import bammodel
import collapsecases as cc
import collapsemodel as m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def col(pkg):
    return importlib.import_module("sicelore_amd.collapsemodel")


def _run(col, ctx, tmp_path, bam, refflat, csv, segment_bytes=256 << 20, **kw):
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bam, block=3000))
    (tmp_path / "r.refFlat").write_text(refflat)
    (tmp_path / "c.csv").write_text(csv)
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    info = col.collapse_model(ctx, str(tmp_path / "in.bam"), str(tmp_path / "r.refFlat"), str(tmp_path / "c.csv"), str(out), prefix="t",
                              segment_bytes=segment_bytes, n_threads=3, host_loop=True, **kw)
    mk = {k: v for k, v in kw.items() if k in ("delta", "min_evidence", "rn_min", "max_clip")}
    want, cnt, _det = m.collapse_model(bam, refflat, csv, **mk)
    names = col.output_names("t", kw.get("delta", 2), kw.get("rn_min", 1), kw.get("min_evidence", 2))
    assert sorted(os.listdir(out)) == sorted(names.values())
    for sfx, data in want.items():
        assert (out / names[sfx]).read_bytes() == data, sfx
    assert {k: info[k] for k in cnt} == cnt
    assert info["host_loop_mismatches"] == 0          # K-COLLAPSE against the single-thread loop of the library, record by record
    return info, cnt


@pytest.mark.parametrize("segment_bytes", [256 << 20, 700])
def test_hand_built_case(col, gpu_ctx, tmp_path, segment_bytes):
    info, cnt = _run(col, gpu_ctx, tmp_path, cc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, segment_bytes=segment_bytes)
    assert cnt["founders"] == 21 and cnt["isoforms"] == 18
    assert (tmp_path / "out" / "t.d2.rn1.e2.txt").read_bytes().count(b"\n") == 19


@pytest.mark.parametrize("kw", [dict(min_evidence=3), dict(min_evidence=4), dict(rn_min=2), dict(delta=0), dict(max_clip=151)], ids=str)
def test_hand_built_case_thresholds(col, gpu_ctx, tmp_path, kw):
    _run(col, gpu_ctx, tmp_path, cc.hand_bam(), cc.HAND_REF, cc.HAND_CSV, **kw)


def test_hand_built_case_other_order(col, gpu_ctx, tmp_path):
    _run(col, gpu_ctx, tmp_path, cc.hand_bam(order_gc2=("a", "b", "c")), cc.HAND_REF, cc.HAND_CSV)


def test_undef_list_sizes(col, gpu_ctx, tmp_path):
    info, cnt = _run(col, gpu_ctx, tmp_path, *cc.sizes_case())
    assert cnt["max_undef"] == cc.BLOCK + 1


def test_founder_counts(col, gpu_ctx, tmp_path):
    info, cnt = _run(col, gpu_ctx, tmp_path, *cc.founders_case())
    assert cnt["max_founders"] == 300


@pytest.mark.parametrize("lds_junc", [cc.LDS_JUNC, 64])
def test_junction_list_lengths(col, gpu_ctx, tmp_path, lds_junc):
    info, cnt = _run(col, gpu_ctx, tmp_path, *cc.junction_lists_case(), lds_junc=lds_junc)
    assert info["long_lists"] == (2 if lds_junc == cc.LDS_JUNC else 4)


def test_filter_list_lengths(col, gpu_ctx, tmp_path):
    info, cnt = _run(col, gpu_ctx, tmp_path, *cc.filter_lists_case())
    assert cnt["novel_filtered"] == len(cc.FILTER_TARGETS)


@pytest.mark.parametrize("kw", [dict(delta=0), dict(delta=2), dict(delta=6000), dict(rn_min=2), dict(rn_min=3), dict(rn_min=4),
                                dict(min_evidence=1), dict(min_evidence=3), dict(delta=-1, min_evidence=1)], ids=str)
def test_seeded_thresholds(col, gpu_ctx, tmp_path, kw):
    _run(col, gpu_ctx, tmp_path, *cc.seeded_case(5), segment_bytes=20000, **kw)


def _cli_fail(pkg, tmp_path, capsys, records, read):
    cli = importlib.import_module("sicelore_amd.cli")
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bammodel.bam_bytes(cc.HEAD, cc.REFS, records), block=3000))
    (tmp_path / "r.refFlat").write_text(cc.HAND_REF)
    (tmp_path / "c.csv").write_text(cc.HAND_CSV)
    out = tmp_path / "out"
    out.mkdir()
    rc = cli.main(["CollapseModel", f"I={tmp_path / 'in.bam'}", f"REFFLAT={tmp_path / 'r.refFlat'}", f"CSV={tmp_path / 'c.csv'}", f"OUTDIR={out}"])
    err = capsys.readouterr().err
    assert rc == 1 and f"read {read}:" in err and os.listdir(out) == []


@pytest.mark.parametrize("which", ["bad_it", "no_it", "zero_line", "int_bc", "z_rn", "z_de", "z_it", "walk"])
def test_loader_errors_exit_1_name_the_read_and_leave_no_file(pkg, gpu_ctx, tmp_path, capsys, which):
    bad = dict(bad_it=cc.rec("bad_it", cc.TA1, "GA", "TA9"), no_it=cc.rec("no_it", cc.TA1, "GA", None), zero_line=cc.rec("zero_line", cc.TA1, "GZ", "TZ0"),
               int_bc=cc.rec("int_bc", cc.TA1, "GA", "TA1", bc=None, extra=cc.tm.aux_int("BC", "C", 3)),
               z_rn=cc.rec("z_rn", cc.TA1, "GA", "TA1", extra=cc.tm.aux_z("RN", "2")), z_de=cc.rec("z_de", cc.TA1, "GA", "TA1", extra=cc.tm.aux_z("de", "0.1")),
               z_it=cc.rec("z_it", cc.TA1, "GA", None, flag=4, extra=cc.tm.aux_int("IT", "C", 1)),     # the casts come first, for an unmapped record too
               walk=cc.rec("walk", [], "GA", "TA1", mapq=0, cigar=[("S", 40)]))[which]               # the walk runs before the filter
    recs = cc.hand_records()
    _cli_fail(pkg, tmp_path, capsys, recs[:30] + [bad] + recs[30:], which)


@pytest.mark.parametrize("which", sorted(cc.BAD_REF_LINES))
def test_bad_refflat_line_exits_1_names_the_line_and_leaves_no_file(pkg, gpu_ctx, tmp_path, capsys, which):
    cli = importlib.import_module("sicelore_amd.cli")
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(cc.hand_bam(), block=3000))
    (tmp_path / "r.refFlat").write_text(cc.bad_refflat(which))
    (tmp_path / "c.csv").write_text(cc.HAND_CSV)
    out = tmp_path / "out"
    out.mkdir()
    rc = cli.main(["CollapseModel", f"I={tmp_path / 'in.bam'}", f"REFFLAT={tmp_path / 'r.refFlat'}", f"CSV={tmp_path / 'c.csv'}", f"OUTDIR={out}"])
    err = capsys.readouterr().err
    assert rc == 1 and f"REFFLAT line {cc.BAD_REF_LINES[which][0]}:" in err and os.listdir(out) == []


def test_isoformmatrix_isobam_then_collapsemodel_through_bin_java(pkg, gpu_ctx, tmp_path):
    """IsoformMatrix ISOBAM=true over a molecule BAM, then CollapseModel on the ISOBAM it wrote, both through bin/java"""
    import tagbammodel as tm

    ref = cc.HAND_REF
    R = []
    for i in range(40):
        junc = (cc.TA1, [(1100, 2500)], [(1100, 3001), (4100, 5001)], cc.TB1)[i % 4]
        pos0, cig = cc.cigar_for(junc, 1000)
        aux = tm.aux_z("BC", f"CELL{i % 3}") + tm.aux_z("U8", f"U{i:04d}") + tm.aux_z("GE", "GB" if i % 4 == 3 else "GA")
        R.append(bammodel.bam_record(f"m{i}", 0, 0, pos0, 60, cig, "ACGT", aux=aux))
    (tmp_path / "mol.bam").write_bytes(bammodel.bgzf_compress(bammodel.bam_bytes(cc.HEAD, cc.REFS, R)))
    (tmp_path / "r.refFlat").write_text(ref)
    (tmp_path / "c.csv").write_text("CELL0\nCELL1\nCELL2\n")
    env = dict(os.environ, PYTHON=sys.executable)
    java = ["bash", os.path.join(ROOT, "sicelore-2.1_amd", "bin", "java"), "-jar", "-Xmx4g", "Jar/Sicelore-2.1.jar"]
    r = subprocess.run(java + ["IsoformMatrix", "-I", "mol.bam", "-REFFLAT", "r.refFlat", "-CSV", "c.csv", "-OUTDIR", ".", "-PREFIX", "s", "-ISOBAM", "true"],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    (tmp_path / "out").mkdir()
    r = subprocess.run(java + ["CollapseModel", "I=s_isobam.bam", "CSV=c.csv", "REFFLAT=r.refFlat", "OUTDIR=out", "PREFIX=CollapseModel"],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "total_isoforms\t\t\t\t4 (40)\t2 (20)" in r.stderr and "Won't perform validation" in r.stderr
    isobam = bammodel.bgzf_decompress((tmp_path / "s_isobam.bam").read_bytes())
    want, cnt, _d = m.collapse_model(isobam, ref, "CELL0\nCELL1\nCELL2\n")
    for sfx, data in want.items():
        assert (tmp_path / "out" / f"CollapseModel.d2.rn1.e2{sfx}").read_bytes() == data, sfx
    assert (cnt["gencode"], cnt["ckj"], cnt["nss"], cnt["undef_records"]) == (2, 1, 1, 20)


def test_seeded_50k_records_chr12_from_this_projects_isobam(pkg, col, gpu_ctx, tmp_path):
    """about 50,000 records of the jittered chr12 fixture of tests/test_isoform_gpu.py through IsoformMatrix ISOBAM=true on the device, then
    CollapseModel on that ISOBAM: most molecules are undef (the jitter of 3 is above DELTA)"""
    from test_isoform_gpu import _chr12, _seeded

    iso = importlib.import_module("sicelore_amd.isoformmatrix")
    bam, csv = _seeded(25000, 7)
    (tmp_path / "mol.bam").write_bytes(bammodel.bgzf_compress(bam, block=0xFF00))
    (tmp_path / "r.refFlat").write_text(_chr12())
    (tmp_path / "c.csv").write_text(csv)
    iso.isoform_matrix(gpu_ctx, str(tmp_path / "mol.bam"), str(tmp_path / "r.refFlat"), str(tmp_path / "c.csv"), str(tmp_path), prefix="s",
                       n_threads=3, isobam=True)
    isobam = bammodel.bgzf_decompress((tmp_path / "s_isobam.bam").read_bytes())
    (tmp_path / "out").mkdir()
    info = col.collapse_model(gpu_ctx, str(tmp_path / "s_isobam.bam"), str(tmp_path / "r.refFlat"), str(tmp_path / "c.csv"), str(tmp_path / "out"),
                              prefix="t", segment_bytes=1 << 20, n_threads=3, host_loop=True)
    want, cnt, _det = m.collapse_model(isobam, _chr12(), csv)
    for sfx, data in want.items():
        assert (tmp_path / "out" / f"t.d2.rn1.e2{sfx}").read_bytes() == data, sfx
    assert {k: info[k] for k in cnt} == cnt and info["host_loop_mismatches"] == 0
    assert cnt["records"] > 45000 and cnt["undef_records"] > cnt["kept"] // 2 and cnt["founders"] > 10000 and cnt["novel_filtered"] > 0
