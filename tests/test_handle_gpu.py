"""What the per-program handles share, through real handles on three-record BAMs of tests/longreadcases.py: the size protocol of a
text getter and the cut of error_read through raw ctypes, close() twice, and an error that names a read whose name is no UTF-8."""
import ctypes
import importlib

import numpy as np
import pytest

import fusionmodel
import longreadcases as lc
import tagbammodel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(pkg):
    return importlib.import_module("sicelore_amd.lib")


def _segment(lib, data):
    bam = np.frombuffer(data, dtype=np.uint8).copy()
    _text, _refs, start = lib.bam_header(bam)
    recs, end = lib.bam_index_records(bam, start, 16)
    assert end == bam.size and recs.size == 3
    return bam, recs


# the middle record fails in every program: RN of type I above 2^31 - 1 (longreadcases "rn_I_2_31")
def _failing(name):
    return lc._one(lc.rec(name, rn=None, extra=tagbammodel.aux_int("RN", "I", 2 ** 31)))


def test_fusion_output_size_protocol(lib, gpu_ctx):
    h = lib.Fusion(gpu_ctx, lc.CSV.encode(), n_threads=2)
    try:
        data = lc.bam([lc.rec("a", ge="GA,GB"), lc.rec("b", ge="GA,GB", umi="V"), lc.rec("c", ge="GA")])
        h.add_segment(*_segment(lib, data))
        outs = h.run()
        assert outs == fusionmodel.fusion_detector(data, lc.CSV)[0] and all(outs.values())
        fn = lib.load_library().smi_fusion_output
        for i, name in enumerate(lib.FUSION_OUTPUTS):
            want = outs[name]
            n = ctypes.c_size_t(12345)
            assert fn(h._h, i, None, 0, ctypes.byref(n)) == 0 and n.value == len(want)            # the size alone
            buf = np.full(len(want) + 1, 0x23, dtype=np.uint8)
            if want:
                n = ctypes.c_size_t(12345)
                assert fn(h._h, i, buf.ctypes.data, len(want) - 1, ctypes.byref(n)) == 1          # one short: 1, the size, nothing written
                assert n.value == len(want) and (buf == 0x23).all()
            n = ctypes.c_size_t(12345)
            assert fn(h._h, i, buf.ctypes.data, len(want), ctypes.byref(n)) == 0 and n.value == len(want)
            assert buf[:-1].tobytes() == want and buf[-1] == 0x23
        n = ctypes.c_size_t(0)
        assert fn(h._h, len(lib.FUSION_OUTPUTS), None, 0, ctypes.byref(n)) != 0
        assert lib.load_library().smi_last_error().decode() == "smi_fusion_output: bad argument"
    finally:
        h.close()
        h.close()                                                      # a second close is harmless
    assert h._h is None


def test_collapse_error_read_cuts_the_name(lib, gpu_ctx):
    h = lib.Collapse(gpu_ctx, b"", lc.CSV.encode(), [r[0] for r in lc.REFS], max_clip=lc.MAX_CLIP, rn_min=lc.RN_MIN, iso_tag="IT", n_threads=2, **lc.TAGS)
    try:
        with pytest.raises(lib.SmiError, match="CollapseModel: read a_long_read_name: "):
            h.add_segment(*_segment(lib, _failing("a_long_read_name")))
        assert h.error_read == ("a_long_read_name", 1)
        fn = lib.load_library().smi_collapse_error_read
        buf, rec = ctypes.create_string_buffer(b"#" * 31), ctypes.c_int64(-7)
        assert fn(h._h, buf, 4, ctypes.byref(rec)) == 0
        assert buf.raw == b"a_l\0" + b"#" * 27 + b"\0" and rec.value == 1
        rec = ctypes.c_int64(-7)
        assert fn(h._h, None, 0, ctypes.byref(rec)) == 0 and rec.value == 1
    finally:
        h.close()
        h.close()
    del h                                                              # (and __del__ after close)


@pytest.mark.parametrize("program", ("fusion", "consensus"))
def test_a_read_name_that_is_no_utf8_still_raises_smi_error(lib, gpu_ctx, program):
    data = _failing("xQy").replace(b"xQy\0", b"x\xffy\0")
    assert data.count(b"x\xffy\0") == 1
    if program == "fusion":
        h = lib.Fusion(gpu_ctx, lc.CSV.encode(), n_threads=2)
    else:
        h = lib.Consensus(gpu_ctx, max_clip=lc.MAX_CLIP, tso_end_tag="TE", polya_start_tag="PS", cdna_tag="CS", us_tag="US", n_threads=2, **lc.TAGS)
    try:
        with pytest.raises(lib.SmiError, match="read x�y: "):
            h.add_segment(*_segment(lib, data))
        if program == "fusion":
            assert h.error_read == ("x�y", 1)
    finally:
        h.close()
        h.close()
