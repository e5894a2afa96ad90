"""K-INFLATE (smi_inflate.hip) on legal DEFLATE that zlib's compressor never writes, and on the streams it must refuse: the catalogue of
tests/deflatecraft.py, whose expected text comes from the writer's own token expander (tests/test_deflate_craft_cpu.py holds zlib's inflater
against it).  One call inflates all legal files; one call holds every illegal file between two good ones; the capacity of a file is a hard
bound on what the kernel writes; 256 members are taken and 257 handed back; members around the 1 MiB CRC piece."""
import ctypes

import numpy as np
import pytest
import torch

import deflatecraft as dc

pytestmark = pytest.mark.gpu

# the kernel's status of a stream (smi_inflate.hip) and what each illegal file of the catalogue must come back with: the refusal has to be the
# one the file was built for -- in particular never "output full" (the file was given room up to its illegal token) and, where the tokens in
# front of the illegal one make text, not the trailer's CRC, which would refuse a decoder that took the token as well
BAD_HEADER, BAD_BLOCK, BAD_CODE, BAD_DISTANCE, OUT_FULL, TRUNCATED, TOO_MANY_MEMBERS, BAD_CRC = range(1, 9)
EXPECTED = {"distance_1_beyond_start": {BAD_DISTANCE}, "distance_into_previous_member": {BAD_DISTANCE}, "fixed_symbol_286": {BAD_CODE},
            "fixed_symbol_287": {BAD_CODE}, "fixed_distance_code_30": {BAD_CODE}, "fixed_distance_code_31": {BAD_CODE},
            "oversubscribed_literal_code": {BAD_CODE}, "incomplete_literal_code_two_codes": {BAD_CODE}, "incomplete_code_length_code": {BAD_BLOCK},
            "missing_end_of_block_code": {BAD_BLOCK}, "hlit_287": {BAD_BLOCK}, "hdist_31": {BAD_BLOCK}, "repeat_16_first": {BAD_BLOCK},
            "repeat_past_the_end": {BAD_BLOCK}, "match_without_distance_code": {BAD_CODE}, "stored_len_nlen_mismatch": {BAD_BLOCK},
            "reserved_block_type": {BAD_BLOCK}, "cut_inside_a_48_bit_token": {TRUNCATED},
            # (the code lengths behind the cut are read from the zero padding: a malformed header or a truncated one)
            "cut_inside_a_dynamic_header": {BAD_BLOCK, TRUNCATED}, "crc_last_byte_of_1048577": {BAD_CRC}, "257_members": {TOO_MANY_MEMBERS}}


@pytest.fixture(scope="module")
def cases(pkg):
    from sicelore_amd import lib as libmod

    return dc.shared_catalogue(lambda text, block_bytes: libmod.bgzf_deflate(text, level=6, block_bytes=block_bytes, n_threads=4))


def _same(name, got, text):
    if got != text:
        k = next((j for j in range(min(len(got), len(text))) if got[j] != text[j]), min(len(got), len(text)))
        raise AssertionError((name, "first difference at byte", k, "of", len(text), got[max(0, k - 20):k + 20], text[max(0, k - 20):k + 20]))


def _run(ctx, cases_, caps):
    """-> {case name: (status, length, members, text)} of one smi_gz_inflate_device call over the cases"""
    out, offs, lens, status, n_mem = ctx.gz_inflate_device([c.file for c in cases_], caps)
    host = out.cpu().numpy()
    return [(int(status[i]), int(lens[i]), int(n_mem[i]), host[offs[i]:offs[i] + min(int(lens[i]), int(caps[i]))].tobytes()) for i in range(len(cases_))]


def _check_legal(cases_, results):
    for c, (status, n, members, got) in zip(cases_, results):
        assert status == 0, (c.name, "status", status, "after", n, "bytes of", len(c.text))
        assert n == len(c.text), (c.name, n, len(c.text))
        _same(c.name, got, c.text)
        assert c.n_members is None or members == c.n_members, (c.name, members)


def test_legal_streams_in_one_call(gpu_ctx, cases):
    legal = [c for c in cases[0] if not c.device_refuses]
    assert len(legal) >= 60
    _check_legal(legal, _run(gpu_ctx, legal, [len(c.text) for c in legal]))


def test_illegal_streams_between_good_neighbours(gpu_ctx, cases):
    """every stream the decoders are specified to refuse comes back with a status, and does nothing to the files around it"""
    legal, illegal = cases
    good = [c for c in legal if c.name in ("one_dist_code/single_1bit", "eob_only/stored_then_match", "dense_steps", "far/stored+fixed", "crc_pieces/257")]
    assert len(good) == 5
    bad = illegal + [c for c in legal if c.device_refuses]
    assert len(bad) >= 21
    batch, caps = [good[0]], [len(good[0].text)]
    for k, c in enumerate(bad):
        g = good[(k + 1) % len(good)]
        batch += [c, g]
        # (room for the text in front of what makes the file illegal, so that it is not the capacity that stops the kernel)
        caps += [len(c.text) if c.text is not None else c.room, len(g.text)]
    results = _run(gpu_ctx, batch, caps)
    assert {c.name.split("/")[1] for c in bad} == set(EXPECTED)
    for c, r in zip(batch, results):
        if c in bad:
            assert r[0] != 0, (c.name, "was inflated", r[:3])
            assert r[0] in EXPECTED[c.name.split("/")[1]], (c.name, "refused with status", r[0], "after", r[1], "bytes")
    _check_legal(batch[0::2], results[0::2])


def test_member_limit(gpu_ctx, cases):
    """256 members are a file's limit (the CRC kernel's table): 255 data blocks and the end-of-file block of a bgzip'd FASTQ go through, 256 do not"""
    a, b = [c for c in cases[0] if c.name.startswith("bgzf_fastq/")]
    assert (a.n_members, b.n_members) == (256, 257) and not a.device_refuses and b.device_refuses
    ra, rb = _run(gpu_ctx, [a, b], [len(a.text), len(b.text)])
    _check_legal([a], [ra])
    assert rb[0] == TOO_MANY_MEMBERS, rb[:3]


def test_crc_pieces(gpu_ctx, cases):
    """members one byte below, at and above the 1 MiB piece of the CRC kernel, of two pieces and one byte, small ones, three in a file; and one
    whose last piece is a single byte with one bit changed"""
    legal, illegal = cases
    mine = [c for c in legal if c.name.startswith("crc_pieces/")]
    wrong = [c for c in illegal if c.name == "illegal/crc_last_byte_of_1048577"]
    assert len(mine) == 9 and len(wrong) == 1
    results = _run(gpu_ctx, mine + wrong, [len(c.text) for c in mine] + [1_048_577])
    _check_legal(mine, results[:-1])
    assert results[-1][0] == BAD_CRC and results[-1][1] == 1_048_577, results[-1][:3]   # (all of it inflated: it is the CRC that refuses it)


def test_capacity_is_a_hard_bound(gpu_ctx, cases):
    """smi_gz_inflate_device as the wrapper calls it, the output prefilled: with the exact capacity the text and nothing behind it; with one
    that is 1, 64 or 300 bytes short a status and nothing from the capacity on (a step of dense_steps has 8 KB to write: the check comes first)"""
    legal = {c.name: c for c in cases[0]}
    picked = [legal["dense_steps"], legal["far/dynamic"], legal["crc_pieces/257"], legal["eob_only/stored_65535_then_match"]]
    files, short = [], []
    for c in picked:
        for s in (0, 1, 64, 300):
            if s < len(c.text):
                files.append(c)
                short.append(s)
    assert len(files) == 15
    in_off, at = [], 0
    for c in files:
        in_off.append(at)
        at = (at + len(c.file) + 511) & ~511
    host = np.zeros(at + 1024, dtype=np.uint8)
    for c, o in zip(files, in_off):
        host[o:o + len(c.file)] = np.frombuffer(c.file, dtype=np.uint8)
    out_off, at = [], 0
    for c in files:
        out_off.append(at)
        at = (at + len(c.text) + 512 + 255) & ~255            # (every file's slot is longer than its text: what is behind a capacity is the slot's own)
    out_off.append(at)
    caps = [len(c.text) - s for c, s in zip(files, short)]
    dev = torch.device("cuda", gpu_ctx.device)
    d_in = torch.from_numpy(host).to(dev)
    d_out = torch.full((at,), 0xA5, dtype=torch.uint8, device=dev)
    n = len(files)
    S = np.zeros((n, 4), dtype=np.uint64)
    S[:, 0], S[:, 1], S[:, 2], S[:, 3] = in_off, [len(c.file) for c in files], out_off[:-1], caps
    R = np.zeros(n, dtype=np.dtype([("out_len", "<u8"), ("status", "<u4"), ("n_members", "<u4")]))
    torch.cuda.synchronize()
    rc = gpu_ctx._lib.smi_gz_inflate_device(gpu_ctx._h, ctypes.c_void_p(d_in.data_ptr()), S.ctypes.data, n, ctypes.c_void_p(d_out.data_ptr()), R.ctypes.data, None)
    assert rc == 0
    got = d_out.cpu().numpy()
    for i, (c, s) in enumerate(zip(files, short)):
        behind = got[out_off[i] + caps[i]:out_off[i + 1]]
        assert (behind == 0xA5).all(), (c.name, "short by", s, "wrote", int(np.nonzero(behind != 0xA5)[0][0]), "bytes behind its capacity")
        if s == 0:
            assert R["status"][i] == 0 and R["out_len"][i] == len(c.text), (c.name, int(R["status"][i]), int(R["out_len"][i]))
            _same(c.name, got[out_off[i]:out_off[i] + caps[i]].tobytes(), c.text)
        else:
            assert R["status"][i] == OUT_FULL, (c.name, "short by", s, int(R["status"][i]))
