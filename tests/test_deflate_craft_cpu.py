"""The host's gzip decoder (smi_inflate_host.hip) on legal DEFLATE that zlib's compressor never writes, and on the streams it must refuse:
the catalogue of tests/deflatecraft.py (distances up to 32768, a single distance code, code-length repeats across the two alphabets, matches
into stored bytes, 15-bit codes and 48-bit tokens, steps of 8 KB, 300 block seams, seeded token mixes, every header field, BGZF, members
around 1 MiB).  zlib's inflater is held against the writer's own token expander first; the project's decoder against the expander's text then,
with the output buffer's end guarded."""
import ctypes
import zlib

import numpy as np
import pytest

import deflatecraft as dc

SHORT = (1, 2, 7, 8, 9, 280)
GUARD = 64


@pytest.fixture(scope="module")
def libmod(pkg):
    from sicelore_amd import lib as libmod

    libmod.load_library()
    return libmod


@pytest.fixture(scope="module")
def cases(libmod):
    return dc.shared_catalogue(lambda text, block_bytes: libmod.bgzf_deflate(text, level=6, block_bytes=block_bytes, n_threads=4))


def test_the_writer_against_zlibs_inflater(cases):
    """zlib's inflater as the independent judge of the writer: every legal stream inflates to the expander's text, every illegal one is refused"""
    legal, illegal = cases
    names = {c.name.split("/")[0] for c in legal}
    assert names == {"far", "one_dist_code", "eob_only", "repeat_across", "deep_codes", "dense_steps", "block_seams", "soup", "headers", "bgzf_fastq", "crc_pieces"}
    for c in legal:
        if c.raw is not None:
            assert zlib.decompress(c.raw, -15) == c.text, c.name
        text, n = dc.gunzip_reference(c.file)
        assert text == c.text and (c.n_members is None or n == c.n_members), (c.name, n)
    assert len(illegal) >= 20
    for c in illegal:
        with pytest.raises(zlib.error):
            dc.gunzip_reference(c.file)
        if c.raw is not None:
            with pytest.raises(zlib.error):
                zlib.decompress(c.raw, -15)


def test_legal_streams_through_gz_inflate(libmod, cases):
    for c in cases[0]:
        got = libmod.gz_inflate(np.frombuffer(c.file, dtype=np.uint8)).tobytes()
        if got != c.text:
            k = next((j for j in range(min(len(got), len(c.text))) if got[j] != c.text[j]), min(len(got), len(c.text)))
            raise AssertionError((c.name, len(got), len(c.text), "first difference at byte", k, got[max(0, k - 20):k + 20], c.text[max(0, k - 20):k + 20]))


def test_capacity_is_a_hard_bound_on_the_host(libmod, cases):
    """smi_gz_inflate into a buffer of exactly the text's size: the text, and not a byte behind it; into one that is a few bytes short
    (inside the reach of the fast loop's 2-byte literal stores, its 8-byte match copies and its 280-byte margin): refused, and not a byte
    from the given capacity on"""
    lib = libmod.load_library()
    for c in cases[0]:
        a = np.frombuffer(c.file, dtype=np.uint8)
        n = len(c.text)
        for short in (0,) + SHORT:
            cap = n - short
            if cap < 0:
                continue
            buf = np.full(n + GUARD, 0xA5, dtype=np.uint8)
            got = ctypes.c_size_t(0)
            rc = lib.smi_gz_inflate(a.ctypes.data, a.size, buf.ctypes.data, cap, ctypes.byref(got))
            assert (buf[cap:] == 0xA5).all(), (c.name, short, "wrote behind the capacity at", cap + int(np.nonzero(buf[cap:] != 0xA5)[0][0]))
            if short == 0:
                assert rc == 0 and got.value == n and buf[:n].tobytes() == c.text, (c.name, rc, got.value)
            else:
                assert rc != 0, (c.name, short)


def test_multi_member_files_step_by_step(libmod, cases):
    """smi_gz_inflate_into: room for all but the last member -> 1 with both positions in front of that member, then the rest"""
    lib = libmod.load_library()
    multi = [c for c in cases[0] if c.n_members and c.n_members > 1]
    assert len(multi) >= 3
    for c in multi:
        a = np.frombuffer(c.file, dtype=np.uint8)
        n = len(c.text)
        buf = np.full(n + GUARD, 0xA5, dtype=np.uint8)
        ip, op = ctypes.c_size_t(0), ctypes.c_size_t(0)
        rc = lib.smi_gz_inflate_into(a.ctypes.data, a.size, ctypes.byref(ip), buf.ctypes.data, n - 1, ctypes.byref(op))
        assert rc == 1 and 0 < op.value < n and c.file[ip.value:ip.value + 3] == b"\x1f\x8b\x08", (c.name, rc, op.value)
        assert buf[:op.value].tobytes() == c.text[:op.value] and (buf[n - 1:] == 0xA5).all(), c.name
        rc = lib.smi_gz_inflate_into(a.ctypes.data, a.size, ctypes.byref(ip), buf.ctypes.data, n, ctypes.byref(op))
        assert rc == 0 and ip.value == a.size and op.value == n and buf[:n].tobytes() == c.text and (buf[n:] == 0xA5).all(), (c.name, rc, op.value)


def test_illegal_streams_are_refused(libmod, cases):
    """... and with the refusal the file was built for: the decoder's three messages are a truncated stream, an invalid DEFLATE stream, and a
    CRC-32 / length that does not match (which would also refuse a decoder that took an illegal token whose file has the empty text's trailer)"""
    for c in cases[1]:
        with pytest.raises(libmod.SmiError) as e:
            libmod.gz_inflate(np.frombuffer(c.file, dtype=np.uint8))
        word = "truncated" if "/cut_inside" in c.name else "CRC-32" if "/crc_" in c.name else "invalid DEFLATE"
        assert word in str(e.value), (c.name, str(e.value))


def _bgzf_block(raw, text, isize=None):
    bsize = 18 + len(raw) + 8
    assert bsize <= 65536 and len(text) <= 65536
    head = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + (bsize - 1).to_bytes(2, "little")
    return head + raw + zlib.crc32(text).to_bytes(4, "little") + (len(text) if isize is None else isize).to_bytes(4, "little")


def test_crafted_payloads_as_bgzf_blocks(libmod):
    """smi_bgzf_inflate (under every BAM read): a block's payload must fill its ISIZE bytes exactly"""
    rng = __import__("random").Random(5)
    far = dc.Fixed(dc._literals(rng, 32768) + dc.FAR_MATCHES, final=True)
    one = dc.Dynamic([65, (258, 1), (258, 1)], dc.lens_of(286, {65: 1, 256: 2, 285: 2}), [1], final=True)
    payloads = [dc.deflate([b]) for b in (far, one, dc.deep_codes_block(n_wide=120), dc.dense_steps_block(n=15))]
    eof = _bgzf_block(b"\x03\x00", b"")
    for raw, text in payloads:
        assert 500 < len(text) < 65536 and zlib.decompress(raw, -15) == text
    file = b"".join(_bgzf_block(raw, text) for raw, text in payloads) + eof
    back, used = libmod.bgzf_inflate(np.frombuffer(file, dtype=np.uint8), n_threads=3)
    assert back.tobytes() == b"".join(t for _, t in payloads) and used == len(file)
    # ISIZE one less than the payload makes: the block does not fit its own size
    raw, text = payloads[3]
    with pytest.raises(libmod.SmiError):
        libmod.bgzf_inflate(np.frombuffer(_bgzf_block(raw, text, isize=len(text) - 1) + eof, dtype=np.uint8), n_threads=1)
    with pytest.raises(libmod.SmiError):
        libmod.bgzf_inflate(np.frombuffer(_bgzf_block(raw, text, isize=len(text) + 1) + eof, dtype=np.uint8), n_threads=1)
