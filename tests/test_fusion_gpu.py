"""FusionDetector on the GPU against tests/fusionmodel.py: the three files byte for byte, every counter the model has and the message
lines, on the hand-built case and the size and key edges of tests/fusioncases.py (tests/test_fusion_cpu.py asserts that each edge is in
its input); the library's single-thread loops must agree with the device molecule by molecule."""
import importlib
import io
import os
import subprocess
import sys

import pytest

import bammodel
import fusioncases as fc
import fusionmodel as m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fd(pkg):
    return importlib.import_module("sicelore_amd.fusiondetector")


def _run(fd, ctx, tmp_path, bam, csv, segment_bytes=256 << 20, block=3000, want=None, **kw):
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bam, block=block))
    (tmp_path / "c.csv").write_text(csv)
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    log = io.StringIO()
    info = fd.fusion_detector(ctx, str(tmp_path / "in.bam"), str(tmp_path / "c.csv"), str(out), prefix="t", segment_bytes=segment_bytes, n_threads=3,
                              host_loop=True, log=log, **kw)
    files, cnt, fusions, _mols = want or m.fusion_detector(bam, csv)
    assert sorted(os.listdir(out)) == sorted("t" + sfx for sfx in m.SUFFIXES)
    for sfx, data in files.items():
        assert (out / ("t" + sfx)).read_bytes() == data, sfx
    assert {k: info[k] for k in cnt} == cnt
    assert info["fusions"] == fusions and log.getvalue().split("\n")[:-1] == m.statistics_lines(cnt, fusions)
    assert info["host_loop_mismatches"] == 0          # the device's grouping against the single-thread loops of the library
    return info, cnt


@pytest.mark.parametrize("segment_bytes", [256 << 20, 700])
def test_hand_built_case(fd, gpu_ctx, tmp_path, segment_bytes):
    info, cnt = _run(fd, gpu_ctx, tmp_path, fc.hand_bam(), fc.HAND_CSV, segment_bytes=segment_bytes, block=600)
    assert cnt["counted"] == 43 and cnt["rows"] == 9 and (tmp_path / "out" / "t_fusmolinfos.txt").read_bytes().count(b"\n") == 44


@pytest.mark.parametrize("case", ["read_sizes", "molecule_sizes", "gene_counts", "keys", "none_counted", "big_row"])
def test_size_and_key_edges(fd, gpu_ctx, tmp_path, case):
    _run(fd, gpu_ctx, tmp_path, *getattr(fc, case + "_case")(), segment_bytes=4000)


def test_no_records(fd, gpu_ctx, tmp_path):
    info, cnt = _run(fd, gpu_ctx, tmp_path, fc.bam([]), fc.CSV5)
    assert info["records"] == 0 and info["bytes_written"] == sum(len(v) for v in m.fusion_detector(fc.bam([]), fc.CSV5)[0].values())


def test_smallest_legal_table_wraps(fd, gpu_ctx, tmp_path):
    """64 records, reads and gene fields in tables of 64 slots: every table ends full, so chains run past the end"""
    info, cnt = _run(fd, gpu_ctx, tmp_path, *fc.tight_table_case(), table_log2=6)
    assert info["wraps"] > 0 and info["probe_steps"] > 0
    lib = importlib.import_module("sicelore_amd.lib")
    with pytest.raises(lib.SmiError, match="table_log2 5 gives a table of fewer slots than the 64 kept records"):
        _run(fd, gpu_ctx, tmp_path, *fc.tight_table_case(), table_log2=5)


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 200])
def test_matrix_rows_under_a_2_kb_render_budget(fd, gpu_ctx, tmp_path, n_rows):
    info, cnt = _run(fd, gpu_ctx, tmp_path, *fc.rows_case(n_rows), budget_bytes=2048)
    # a row takes 5 x 4 bytes of counts, 26 of label, 5 x 2 of text, 1 + 8: 65 bytes, 31 rows to a block
    assert cnt["rows"] == n_rows and info["render_blocks"] == -(-n_rows // 31)


def test_seeded_20k_records_in_segments_twice(fd, gpu_ctx, tmp_path):
    bam, csv = fc.seeded_case(3)
    want = m.fusion_detector(bam, csv)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    info, cnt = _run(fd, gpu_ctx, tmp_path / "a", bam, csv, segment_bytes=100000, block=0xFF00, want=want)
    _run(fd, gpu_ctx, tmp_path / "b", bam, csv, segment_bytes=30000, block=0xFF00, want=want)
    for sfx in m.SUFFIXES:
        assert (tmp_path / "a" / "out" / ("t" + sfx)).read_bytes() == (tmp_path / "b" / "out" / ("t" + sfx)).read_bytes()
    assert cnt["records"] > 19000 and cnt["molecules"] > 2000 and cnt["counted"] > 50


BAD = dict(int_bc=lambda: fc.rec("int_bc", "GA", bc=None, extra=fc.tm.aux_int("BC", "C", 3)),
           int_u8=lambda: fc.rec("int_u8", "GA", umi=None, extra=fc.tm.aux_int("U8", "C", 3)),
           int_ge=lambda: fc.rec("int_ge", None, flag=4, extra=fc.tm.aux_int("GE", "C", 3)),         # the casts come first, for an unmapped record too
           z_rn=lambda: fc.rec("z_rn", "GA", extra=fc.tm.aux_z("RN", "2")),
           z_de=lambda: fc.rec("z_de", "GA", df=0.1, extra=fc.tm.aux_z("de", "0.1")),
           z_df=lambda: fc.rec("z_df", "GA", extra=fc.tm.aux_z("df", "0.1")),
           walk=lambda: fc.rec("walk", "undef", cigar=[("S", 40)]),                                    # the walk runs before the filter
           no_cigar=lambda: fc.rec("no_cigar", "GA", cigar=[]))


@pytest.mark.parametrize("which", sorted(BAD))
def test_parse_errors_exit_1_name_the_read_and_leave_no_file(pkg, gpu_ctx, tmp_path, capsys, which):
    cli = importlib.import_module("sicelore_amd.cli")
    recs = fc.hand_records()
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(fc.bam(recs[:30] + [BAD[which]()] + recs[30:]), block=600))
    (tmp_path / "c.csv").write_text(fc.HAND_CSV)
    out = tmp_path / "out"
    out.mkdir()
    rc = cli.main(["FusionDetector", f"I={tmp_path / 'in.bam'}", f"CSV={tmp_path / 'c.csv'}", f"O={out}"])
    err = capsys.readouterr().err
    assert rc == 1 and f"read {which}:" in err and os.listdir(out) == []


def test_records_the_parser_never_casts(fd, gpu_ctx, tmp_path):
    """RN, de and the CIGAR of an unmapped record, and df behind a float de, are not looked at"""
    ok = [fc.rec("a", "GA", flag=4, cigar=[], extra=fc.tm.aux_z("RN", "2") + fc.tm.aux_z("de", "x")), fc.rec("b", "GA,GB", de=0.5, extra=fc.tm.aux_z("df", "x"))]
    info, cnt = _run(fd, gpu_ctx, tmp_path, fc.bam(ok), "CELL1\n")
    assert cnt["valid"] == 1 and cnt["counted"] == 1


def test_readme_step_6_line_through_bin_java(pkg, gpu_ctx, tmp_path):
    """the reference README's step 6 line, verbatim"""
    (tmp_path / "clipped_reads.tags.US.bam").write_bytes(bammodel.bgzf_compress(fc.hand_bam()))
    (tmp_path / "ValidBarcodes.csv").write_text(fc.HAND_CSV)
    env = dict(os.environ, PYTHON=sys.executable)
    java = ["bash", os.path.join(ROOT, "sicelore-2.1_amd", "bin", "java"), "-jar", "-Xmx4g", "Jar/Sicelore-2.1.jar"]
    r = subprocess.run(java + "FusionDetector I=clipped_reads.tags.US.bam O=. PREFIX=fusion CSV=ValidBarcodes.csv".split(),
                       env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    files, cnt, fusions, _mols = m.fusion_detector(fc.hand_bam(), fc.HAND_CSV)
    for sfx, data in files.items():
        assert (tmp_path / ("fusion" + sfx)).read_bytes() == data, sfx
    lines = r.stderr.split("\n")
    want = m.statistics_lines(cnt, fusions)
    at = lines.index(want[0])
    assert lines[at:at + len(want)] == want and "\t10 distincts molecules support fusion [F1|F2]" in lines
