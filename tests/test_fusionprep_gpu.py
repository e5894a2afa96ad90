"""ExportClippedReads (K-CLIP-*: smi_clipexport.hip) and AddBamReadTags (K-NAME's '_' form + K-EDIT: smi_moltag.hip) on the GPU against
tests/fusionprepmodel.py: the FASTQ and the BAM byte for byte, every counter the model has, the read a stopped run names, the library's
single-thread loop record by record, and the reference README's step 6 as a chain of processes.  tests/test_fusionprep_cpu.py asserts
that each edge named here is in its input."""
import importlib
import os
import subprocess
import sys

import pytest

import bammodel
import fusionprepcases as pc
import fusionprepmodel as m
import moltagcases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSIONPREP = os.path.join(ROOT, "sicelore-2.1_amd", "fusionprep.py")


@pytest.fixture(scope="module")
def fp(pkg):
    return importlib.import_module("sicelore_amd.fusionprep")


@pytest.fixture(scope="module")
def lib(pkg):
    return importlib.import_module("sicelore_amd.lib")


def _export(fp, ctx, tmp_path, bam, block=0xFF00, segment_bytes=256 << 20, want=None, **kw):
    tmp_path.mkdir(exist_ok=True)
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bam, block=block))
    dst = tmp_path / "out.fastq"
    info = fp.export_clipped_reads(ctx, str(tmp_path / "in.bam"), str(dst), segment_bytes=segment_bytes, n_threads=3, host_loop=True, **kw)
    model_kw = {k: v for k, v in kw.items() if k != "table_log2"}
    fastq, cnt, _dec = want or m.export_clipped_reads(bam, **model_kw)
    assert dst.read_bytes() == fastq and sorted(os.listdir(tmp_path)) == ["in.bam", "out.fastq"]
    assert {k: info[k] for k in cnt} == cnt and info["bytes_written"] == len(fastq)
    assert info["host_loop_mismatches"] == 0            # the device's decisions against the single-thread loop of the library
    return info


def _tags(fp, ctx, tmp_path, bam, block=0xFF00, segment_bytes=256 << 20, **tags):
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bam, block=block))
    dst = tmp_path / "out.bam"
    info = fp.add_bam_read_tags(ctx, str(tmp_path / "in.bam"), str(dst), segment_bytes=segment_bytes, **tags)
    want, cnt = m.add_bam_read_tags(bam, tags.get("gene_tag", "GE"), tags.get("cell_tag", "BC"), tags.get("umi_tag", "U8"))
    raw = dst.read_bytes()
    assert raw.endswith(bammodel.bgzf_block(b"")) and bammodel.bgzf_decompress(raw) == want
    assert {k: info[k] for k in cnt} == cnt
    return info


# ---- ExportClippedReads -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segmented", [False, True])
def test_hand_built_case(fp, gpu_ctx, tmp_path, segmented):
    info = _export(fp, gpu_ctx, tmp_path, pc.hand_bam(), block=600 if segmented else 0xFF00, segment_bytes=700 if segmented else 256 << 20)
    assert (info["records"], info["clipped"], info["written"]) == (32, 25, 21) and (info["segments"] > 1) == segmented


def test_options(fp, gpu_ctx, tmp_path):
    for k, mc_ in enumerate((149, 200, -1, 2 ** 31 - 1, -2 ** 31)):
        _export(fp, gpu_ctx, tmp_path / f"m{k}", pc.hand_bam(), min_clip=mc_)
    _export(fp, gpu_ctx, tmp_path / "t1", pc.hand_bam(), gene_tag="BC", cell_tag="BC", umi_tag="BC", us_tag="QS", qs_tag="QS")
    _export(fp, gpu_ctx, tmp_path / "t2", pc.hand_bam(), gene_tag="U8", cell_tag="GE", umi_tag="XX", us_tag="BC", qs_tag="US")


@pytest.mark.parametrize("segment_bytes", [256 << 20, 20000])
def test_sequence_lengths_at_every_alignment(fp, gpu_ctx, tmp_path, segment_bytes):
    info = _export(fp, gpu_ctx, tmp_path, pc.lengths_case(), segment_bytes=segment_bytes, block=4096)
    assert info["written"] == 48


@pytest.mark.parametrize("segment_bytes", [256 << 20, 1500])
def test_one_key_many_times(fp, gpu_ctx, tmp_path, segment_bytes):
    """1 / 2 / 63 / 64 / 65 records of a key inside one segment, and spread over three segments or more"""
    info = _export(fp, gpu_ctx, tmp_path, pc.dup_case(), segment_bytes=segment_bytes, block=1200)
    assert info["written"] == 5 and (info["segments"] >= 3 or segment_bytes > 1500)


@pytest.mark.parametrize("segment_bytes", [256 << 20, 900])
def test_prefix_keys_and_last_byte(fp, gpu_ctx, tmp_path, segment_bytes):
    _export(fp, gpu_ctx, tmp_path, pc.prefix_case(), segment_bytes=segment_bytes, block=700)


def test_table_ends_exactly_half_full(fp, gpu_ctx, tmp_path):
    info = _export(fp, gpu_ctx, tmp_path, pc.distinct_case(64, dups=False), table_log2=7)
    assert (info["written"], info["table_slots"], info["table_grows"]) == (64, 128, 0)


def test_table_grows_and_chains_wrap(fp, gpu_ctx, tmp_path):
    """200 distinct keys, three of them with the last slot as their home, over four segments or more from a table of 16 slots"""
    bam = pc.distinct_case(200, wrap=3)
    info = _export(fp, gpu_ctx, tmp_path, bam, table_log2=4, block=4096, segment_bytes=len(bammodel.bgzf_compress(bam, block=4096)) // 4)
    assert info["written"] == 200 and info["segments"] >= 4 and info["table_grows"] >= 2 and info["table_slots"] >= 512
    assert info["wraps"] > 0 and info["probe_steps"] > 0


def test_nothing_clipped_and_no_record(fp, gpu_ctx, tmp_path):
    info = _export(fp, gpu_ctx, tmp_path / "a", pc.none_clipped_case())
    assert (info["records"], info["bytes_written"]) == (100, 0)
    info = _export(fp, gpu_ctx, tmp_path / "b", pc.bam([]))
    assert (info["records"], info["bytes_written"]) == (0, 0)
    info = _tags(fp, gpu_ctx, tmp_path, pc.bam([]))
    assert info["records"] == 0 and bammodel.bgzf_decompress((tmp_path / "out.bam").read_bytes()) == pc.bam([])


@pytest.mark.parametrize("which,read", [("underscores", "___"), ("a_typed_bc", "abc"), ("h_typed_us", "hus"), ("int_typed_qs", "iqs"),
                                        ("no_cigar", "nocigar"), ("eq_clip", "eqclip"), ("eq_clip_2", "eqclip2")])
@pytest.mark.parametrize("segmented", [False, True])
def test_stop_cases_exit_1_name_the_read_and_leave_no_file(fp, lib, gpu_ctx, tmp_path, capsys, which, read, segmented):
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(pc.stop_bam(which), block=600 if segmented else 0xFF00))
    src, dst = str(tmp_path / "in.bam"), str(tmp_path / "out.fastq")
    if segmented:
        with pytest.raises(lib.ClipExportError) as e:
            fp.export_clipped_reads(gpu_ctx, src, dst, segment_bytes=700)
        assert (e.value.read, e.value.record) == (read, 20) and f"read {read}:" in str(e.value)
    else:
        assert fp.main(["ExportClippedReads", f"I={src}", f"O={dst}"]) == 1
        err = capsys.readouterr().err
        assert f"read {read}:" in err and "record 20" in err
    assert os.listdir(tmp_path) == ["in.bam"]                     # no output file, no temporary file


def test_damaged_attributes_are_refused_and_leave_no_file(fp, lib, gpu_ctx, tmp_path):
    """every way an attribute list goes wrong (tests/auxcases.py DAMAGED) under K-CLIP-FLAG's walk"""
    for name, bam in pc.damaged_cases().items():
        (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bam))
        with pytest.raises(lib.SmiError, match="a record's attributes cannot be read: malformed or unknown attribute type"):
            fp.export_clipped_reads(gpu_ctx, str(tmp_path / "in.bam"), str(tmp_path / "out.fastq"))
        assert os.listdir(tmp_path) == ["in.bam"], name


def test_a_stop_behind_a_written_record_of_its_key_is_none(fp, gpu_ctx, tmp_path):
    R = pc.hand_records()
    _export(fp, gpu_ctx, tmp_path, pc.bam(R + [pc.rec("hus_first", pc.S200, ge="GH"), pc.STOPS["h_typed_us"]()]), block=600, segment_bytes=700)


def test_seeded_20k_records_in_segments_twice(fp, gpu_ctx, tmp_path):
    bam = pc.seeded_case(5)
    want = m.export_clipped_reads(bam)
    a = _export(fp, gpu_ctx, tmp_path / "a", bam, segment_bytes=100000, want=want)
    b = _export(fp, gpu_ctx, tmp_path / "b", bam, segment_bytes=30000, want=want)
    assert (tmp_path / "a" / "out.fastq").read_bytes() == (tmp_path / "b" / "out.fastq").read_bytes()
    assert a["segments"] > 3 and b["segments"] > a["segments"] and a["written"] > 2000


# ---- AddBamReadTags ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segmented", [False, True])
def test_read_names_match_the_model(fp, gpu_ctx, tmp_path, segmented):
    info = _tags(fp, gpu_ctx, tmp_path, pc.bam(pc.read_records() * (4 if segmented else 1)), block=500 if segmented else 0xFF00,
                 segment_bytes=600 if segmented else 256 << 20)
    assert info["tagged"] == 8 * (4 if segmented else 1)


def test_read_tag_options_may_coincide(fp, gpu_ctx, tmp_path):
    for opt in (dict(gene_tag="XX", cell_tag="XX", umi_tag="YY"), dict(gene_tag="XX", cell_tag="YY", umi_tag="XX"), dict(gene_tag="XX", cell_tag="XX", umi_tag="XX"),
                dict(gene_tag="NM", cell_tag="AA", umi_tag="ZZ")):
        _tags(fp, gpu_ctx, tmp_path, pc.read_bam(), **opt)


def test_molecule_program_is_unchanged_beside_it(pkg, gpu_ctx, tmp_path):
    import moltagmodel as mm
    mt = importlib.import_module("sicelore_amd.moltags")
    bam = mc.bam_of([("chr1", 10 ** 6)], mc.name_records())
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(bam))
    info = mt.add_bam_molecule_tags(gpu_ctx, str(tmp_path / "in.bam"), str(tmp_path / "out.bam"))
    want, cnt = mm.add_molecule_tags(bam)
    assert bammodel.bgzf_decompress((tmp_path / "out.bam").read_bytes()) == want and info["tagged"] == cnt["tagged"]


def test_read_tags_attribute_limit(fp, lib, gpu_ctx, tmp_path):
    fits = [mc.rec("g_c_u", [("M", 4)], aux=mc.many_attrs(61)), mc.rec("plain", [("M", 4)], aux=mc.many_attrs(64))]
    _tags(fp, gpu_ctx, tmp_path, pc.bam(fits))
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(pc.bam(fits + [mc.rec("g_c_u", [("M", 4)], aux=mc.many_attrs(62))])))
    os.remove(tmp_path / "out.bam")
    with pytest.raises(lib.SmiError, match="more than 64 attributes"):
        fp.add_bam_read_tags(gpu_ctx, str(tmp_path / "in.bam"), str(tmp_path / "out.bam"))
    assert os.listdir(tmp_path) == ["in.bam"]


# ---- the reference README's step 6 ------------------------------------------------------------------------------------------------------
def test_readme_step_6_as_a_chain_of_processes(pkg, tmp_path):
    """ExportClippedReads -> (the test maps: one record per FASTQ name) -> AddBamReadTags -> FusionDetector, each its own process"""
    import fusionmodel as fm

    bam = pc.bam(pc.chain_records())
    (tmp_path / "passedParsedWithSequences.bam").write_bytes(bammodel.bgzf_compress(bam))
    (tmp_path / "ValidBarcodes.csv").write_text(pc.CHAIN_CSV)
    env = dict(os.environ, PYTHON=sys.executable)
    env.pop("WORLD_SIZE", None)

    def run(cmd):
        r = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r

    run([sys.executable, FUSIONPREP] + "ExportClippedReads I=passedParsedWithSequences.bam O=clipped_reads.fastq".split())
    fastq, cnt, _dec = m.export_clipped_reads(bam)
    assert (tmp_path / "clipped_reads.fastq").read_bytes() == fastq and cnt["written"] == 48
    (tmp_path / "clipped_reads.bam").write_bytes(bammodel.bgzf_compress(pc.remapped_bam(fastq)))
    run([sys.executable, FUSIONPREP] + "AddBamReadTags I=clipped_reads.bam O=clipped_reads.tags.bam".split())
    tagged, _cnt = m.add_bam_read_tags(pc.remapped_bam(fastq))
    assert bammodel.bgzf_decompress((tmp_path / "clipped_reads.tags.bam").read_bytes()) == tagged
    os.replace(tmp_path / "clipped_reads.tags.bam", tmp_path / "clipped_reads.tags.US.bam")     # (AddBamReadSequenceTag: FusionDetector reads no US)
    java = ["bash", os.path.join(ROOT, "sicelore-2.1_amd", "bin", "java"), "-jar", "-Xmx32g", "sicelore-2.1.jar"]
    run(java + "FusionDetector I=clipped_reads.tags.US.bam O=. PREFIX=fusion CSV=ValidBarcodes.csv".split())
    files, fc, fusions, _mols = fm.fusion_detector(tagged, pc.CHAIN_CSV)
    for sfx, data in files.items():
        assert (tmp_path / ("fusion" + sfx)).read_bytes() == data, sfx
    assert dict(fusions) == {"BCR|ABL1": 12}
