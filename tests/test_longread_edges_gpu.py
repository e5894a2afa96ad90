"""The BAMs of tests/longreadcases.py through the four real handles (smi_isoform_*, smi_consensus_*, smi_collapse_*, smi_fusion_*):
add_segment, the record-level counters and the read an error names against the Python models.  Only the public ABI is touched and no
handle is run, so no kernel is launched."""
import importlib

import numpy as np
import pytest

import bammodel
import longreadcases as lc

pytestmark = pytest.mark.gpu
WHO = dict(isoform="IsoformMatrix", consensus="ComputeConsensus", collapse="CollapseModel", fusion="FusionDetector")


@pytest.fixture(scope="module")
def lib(pkg):
    return importlib.import_module("sicelore_amd.lib")


@pytest.fixture(scope="module")
def want():
    """the models' reading of every case, computed once"""
    return {name: lc.expected(name) for name in lc.CASES}


def _handle(lib, ctx, program):
    tags = dict(lc.TAGS, n_threads=4)
    if program == "isoform":
        return lib.Isoform(ctx, b"", lc.CSV.encode(), max_clip=lc.MAX_CLIP, **tags)
    if program == "consensus":
        return lib.Consensus(ctx, max_clip=lc.MAX_CLIP, tso_end_tag="TE", polya_start_tag="PS", cdna_tag="CS", us_tag="US", **tags)
    if program == "collapse":
        return lib.Collapse(ctx, b"", lc.CSV.encode(), [r[0] for r in lc.REFS], max_clip=lc.MAX_CLIP, rn_min=lc.RN_MIN, iso_tag="IT", **tags)
    return lib.Fusion(ctx, lc.CSV.encode(), n_threads=4)


@pytest.mark.parametrize("program", lc.PROGRAMS)
@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_the_handle_reads_the_case_as_its_model_does(lib, gpu_ctx, want, name, program):
    data, kw = lc.CASES[name]
    w = want[name][program]
    bam = np.frombuffer(data, dtype=np.uint8).copy()
    _text, _refs, start = lib.bam_header(bam)
    recs, end = lib.bam_index_records(bam, start, 10000)
    assert end == bam.size
    if "outside" in kw:
        recs["aux_off"][kw["outside"]] = bam.size - recs["aux_len"][kw["outside"]] + 1
    h = _handle(lib, gpu_ctx, program)
    try:
        if w[0] == "counts":
            h.add_segment(bam, recs)
            got = h.counts()
            assert {k: got[k] for k in lc.COUNTS[program]} == w[1]
            return
        with pytest.raises(lib.SmiError) as e:
            h.add_segment(bam, recs)
        msg = str(e.value)
        assert h.counts()["records"] == 0                             # a failed segment counts nothing
        if w[0] == "refused":
            assert msg == f"smi_{program}_add_segment: record {w[1]} lies outside the segment"
            return
        assert msg.startswith(f"{WHO[program]}: read {w[1]}: "), msg
        if program == "consensus" or w[2] in (lc.MALFORMED, "no CIGAR", "the CIGAR walk runs past the alignment blocks"):
            assert msg == f"{WHO[program]}: read {w[1]}: {w[2]}"      # (the other models word a failed cast in their own way)
        if program in ("collapse", "fusion"):
            names = [r["name"] for r in bammodel.parse_bam(data)[2]]
            assert h.error_read == (w[1], names.index(w[1]))
    finally:
        h.close()
