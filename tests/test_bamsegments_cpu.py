"""The BAM reader of the file programs (sicelore-2.1_amd/bamsegments.py) on its own: its calls are host functions, so it runs on a CPU.
A BAM of two references and six records, compressed in BGZF blocks of 64 bytes so that the header and the records straddle blocks, is
read with segment sizes from 5 bytes to more than the file: the header comes once, with the first item, and the records are the file's,
in order, whatever the size.  A file cut inside a block, a record cut short and a file without a (whole) header fail by name."""
import importlib
import struct

import pytest

import __graft_entry__ as graft
import bammodel

HEADER_TEXT = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chrUn_KI270442v1\tLN:500\n"
REFS = [("chr1", 1000), ("chrUn_KI270442v1", 500)]
RECORDS = [
    bammodel.bam_record("r0", 0, 0, 10, 30, [("M", 4)], "ACGT", aux=b"BCZAAAC\0"),
    bammodel.bam_record("r1", 16, 0, 20, 0, [("S", 2), ("M", 6)], "ACGTACGT", bytes(range(8))),
    bammodel.bam_record("a_read_with_a_name_longer_than_one_block_of_sixty_four_bytes_0123456789_0123456789", 0, 1, 30, 60, [("M", 3)], "ACG"),
    bammodel.bam_record("r3", 4, -1, -1, 0, [], "ACGTA"),
    bammodel.bam_record("r4", 0, 1, 40, 9, [("M", 2), ("N", 100), ("M", 2)], "ACGT", aux=b"U8ZTTTT\0RNi" + struct.pack("<i", 3)),
    bammodel.bam_record("r5", 256, 0, 50, 1, [("M", 1)], "A"),
]
BAM = bammodel.bam_bytes(HEADER_TEXT, REFS, RECORDS)
HEADER = bammodel.bam_bytes(HEADER_TEXT, REFS, [])
FILE = bammodel.bgzf_compress(BAM, block=64)
SIZES = (5, 64, len(FILE) - 1, len(FILE), 1 << 20)


@pytest.fixture(scope="module")
def segments(pkg):
    return importlib.import_module(graft.PKG_NAME + ".bamsegments").segments


def _write(tmp_path, data):
    p = tmp_path / "in.bam"
    p.write_bytes(data)
    return str(p)


def _records(items):
    """every yielded record as (name, flag, ref_id, pos, mapq, record bytes)"""
    out = []
    for bam, recs, _hdr in items:
        for r in recs:
            o, n = int(r["rec_off"]), int(r["rec_len"])
            name = bam[int(r["name_off"]):int(r["name_off"]) + int(r["l_read_name"]) - 1].tobytes().decode()
            out.append((name, int(r["flag"]), int(r["ref_id"]), int(r["pos"]), int(r["mapq"]), bam[o:o + n].tobytes()))
    return out


def test_the_input_straddles_blocks():
    assert len(HEADER) > 64 and any(len(r) > 64 for r in RECORDS) and len(FILE) > 20 * 64 // 2


@pytest.mark.parametrize("segment_bytes", SIZES)
def test_header_once_and_the_records_in_order(segments, tmp_path, segment_bytes):
    path = _write(tmp_path, FILE)
    items = list(segments(path, segment_bytes, 2))
    assert [hdr is not None for _bam, _recs, hdr in items] == [True] + [False] * (len(items) - 1)
    assert items[0][2] == HEADER
    _text, _refs, want = bammodel.parse_bam(BAM)
    got = _records(items)
    assert [g[0] for g in got] == [w["name"] for w in want]
    assert [g[1:5] for g in got] == [(w["flag"], w["ref_id"], w["pos0"], w["mapq"]) for w in want]
    assert b"".join(g[5] for g in got) == BAM[len(HEADER):]
    secs = dict(bam_read_inflate=1.0, index=2.0, other=3.0)
    assert _records(segments(path, segment_bytes, 2, secs)) == got
    assert sorted(secs) == ["bam_read_inflate", "index", "other"] and secs["other"] == 3.0
    assert secs["bam_read_inflate"] > 1.0 and secs["index"] > 2.0


@pytest.mark.parametrize("segment_bytes", SIZES)
def test_failures_name_the_file(pkg, segments, tmp_path, segment_bytes):
    def fails(data):
        path = _write(tmp_path, data)
        with pytest.raises(pkg.SmiError) as e:
            list(segments(path, segment_bytes, 2))
        return str(e.value), path

    cut = len(FILE) - 28 - 10                    # inside the last block in front of the end-of-file block
    text, path = fails(FILE[:cut])
    assert text == f"{path}: truncated BGZF stream"
    text, path = fails(bammodel.bgzf_compress(BAM[:-3], block=64))
    assert text == f"{path}: truncated BAM record"
    # no header at all, and half of one: smi_bam_header's own texts, as before the reader was shared
    assert fails(b"")[0] == "smi_bam_header: not a BAM stream (magic)"
    assert fails(bammodel.bgzf_compress(b"", block=64))[0] == "smi_bam_header: not a BAM stream (magic)"
    assert fails(bammodel.bgzf_compress(HEADER[:len(HEADER) // 2], block=64))[0] == "smi_bam_header: truncated header text"


def test_a_header_cut_in_its_reference_list(pkg, segments, tmp_path):
    path = _write(tmp_path, bammodel.bgzf_compress(HEADER[:-6], block=64))
    with pytest.raises(pkg.SmiError) as e:
        list(segments(path, 64, 2))
    assert str(e.value) == "smi_bam_header: truncated reference list"
