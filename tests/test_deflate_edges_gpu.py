"""K-DEFLATE (smi_deflate.hip) held to the byte-exact model of tests/deflateread.py over the edge cases of tests/deflateedges.py: the header's
zero-run tokens at every critical length and seam, ties and small alphabets, full blocks that must come out optimal and full blocks that
must be flattened, sizes around the 64-byte runs and the places where their owner starts over, input pointers of every alignment, BGZF,
and block slots that held other bits before.  For every output: zlib inflates it to the input; the reader accounts for every bit; the
output EQUALS the model's bytes for the code lengths found in it (the only thing taken from the device); those lengths are a complete,
ordered code of at most 15 bits that costs what the case demands (deflateedges.check_stream).

What the four flattened blocks cost on the device is recorded in profiles/deflate_edges/README.md; the assertion is the analytic bound of
deflateedges.check_lengths, not the recorded figure."""
import gzip

import numpy as np
import pytest
import torch

import deflateedges as de
import deflateread as dr

pytestmark = pytest.mark.gpu


def _on_device(ctx, data, off=0):
    """the bytes on the device, `off` bytes into an allocation of their own (an unaligned view for off % 16 != 0)"""
    dev = torch.device("cuda", ctx.device)
    if not len(data) and not off:
        return torch.zeros(0, dtype=torch.uint8, device=dev)
    return torch.from_numpy(np.frombuffer(b"\xEE" * off + bytes(data), dtype=np.uint8).copy()).to(dev)[off:]


def _deflate(ctx, data, raw=False, off=0):
    return ctx.gzip_device(_on_device(ctx, data, off), len(data), raw_deflate=raw).cpu().numpy().tobytes()


def _both(ctx, name, text, must=None):
    """gzip and raw of one text through the whole comparison -> the figures of the gzip run"""
    z = _deflate(ctx, text)
    figs = de.check_stream(name, z, text, "gzip", must=must)
    r = _deflate(ctx, text, raw=True)
    de.check_stream(name, r, text, "raw", must=must)
    assert r == z[10:-8], (name, "the raw stream is not the member's")
    return figs


@pytest.fixture(scope="module")
def small():
    return de.small_cases()


@pytest.mark.parametrize("family", ["gap/", "one_byte/", "two_bytes/", "every_", "all_256"])
def test_zero_runs_of_the_header(gpu_ctx, small, family):
    cases = [c for c in small if c.name.startswith(family)]
    assert cases
    for c in cases:
        _both(gpu_ctx, c.name, c.text, [c.must])


@pytest.mark.parametrize("part", range(4))
def test_ties_and_small_alphabets(gpu_ctx, small, part):
    """at most 2048 bytes: no code is 16 deep, nothing may be flattened, the cost is the Huffman cost"""
    cases = [c for c in small if c.name.startswith("ties/")][part::4]
    assert len(cases) == 50
    for c in cases:
        _both(gpu_ctx, c.name, c.text, [c.must])


def test_full_blocks_optimal_and_flattened(gpu_ctx):
    """the blocks of one member, 64 KiB each but the last: those of the two families that cannot be 16 deep cost the Huffman cost; the
    four no Huffman code of which fits 15 bits lie between the package-merge optimum and the bound of the halving rule"""
    full = de.full_blocks()
    text = b"".join(c.text for c in full)
    figs = _both(gpu_ctx, "full", text, [c.must for c in full])
    assert [f["must"] for f in figs].count("flat") == 4
    for c, f in zip(full, figs):
        if c.must == "flat":
            print(f"K-DEFLATE flattened {c.name}: device {f['cost']} bits, package-merge {f['optimum']}, bound {f['bound']}, "
                  f"excess {f['excess']} ({100.0 * f['excess'] / f['optimum']:.4f} %)")


@pytest.mark.parametrize("n", de.SEAM_SIZES)
def test_seams_of_runs_owners_and_blocks(gpu_ctx, n):
    """sizes around the 64-byte runs, around 16384 / 32768 / 49152 bytes (the thread that owns a run starts over) and around the block,
    from an aligned input pointer and from unaligned ones (the byte-wise path): the same bytes whatever the alignment"""
    text = de.seam_text(n)
    first = None
    for off in de.SEAM_OFFSETS:
        z = _deflate(gpu_ctx, text, off=off)
        de.check_stream(f"seam/{n}@{off}", z, text, "gzip")
        first = z if first is None else first
        assert z == first, (n, off, "the output depends on the input pointer's alignment")
        assert _deflate(gpu_ctx, text, raw=True, off=off) == z[10:-8], (n, off, "raw")


def test_bgzf_long_runs(gpu_ctx):
    for c in de.long_run_cases():
        z = gpu_ctx.bgzf_deflate_device(c.text).tobytes()
        de.check_stream(c.name, z, c.text, "bgzf", de.BGZF_IN, [c.must])


@pytest.mark.parametrize("n", de.BGZF_SIZES)
def test_bgzf_sizes_around_its_blocks(gpu_ctx, n):
    """BSIZE, CRC-32 and ISIZE of every block and the 28-byte end-of-file block are the model's"""
    text = de.seam_text(n)
    de.check_stream(f"bgzf/{n}", gpu_ctx.bgzf_deflate_device(text).tobytes(), text, "bgzf", de.BGZF_IN)


def test_block_slots_that_held_other_bits(gpu_ctx, small):
    """the context's scratch is reused from call to call: after an incompressible input has left dense bits in every slot, the same cases give
    the same bytes (a slot word nobody writes would show now)"""
    cases = [c for c in small if c.name in ("gap/63+2", "one_byte/138", "ties/3_4lit", "all_256")] + [de.Edge("seam/65473", de.seam_text(65473)),
                                                                                                          de.Edge("seam/131137", de.seam_text(65536 + 65))]
    assert len(cases) == 6
    before = [(_deflate(gpu_ctx, c.text), _deflate(gpu_ctx, c.text, raw=True), gpu_ctx.bgzf_deflate_device(c.text).tobytes()) for c in cases]
    dense = np.random.default_rng(300).integers(0, 256, size=300_000, dtype=np.uint8).tobytes()
    dense_z = _deflate(gpu_ctx, dense)
    de.check_stream("dense", dense_z, dense, "gzip")
    dense_b = gpu_ctx.bgzf_deflate_device(dense).tobytes()
    for c, (z, r, b) in zip(cases, before):
        assert _deflate(gpu_ctx, dense) == dense_z
        assert _deflate(gpu_ctx, c.text) == z, c.name
        de.check_stream(c.name, z, c.text, "gzip", must=[c.must] if c.must else None)
        assert _deflate(gpu_ctx, dense, raw=True) == dense_z[10:-8]
        assert _deflate(gpu_ctx, c.text, raw=True) == r == z[10:-8], c.name
        assert _deflate(gpu_ctx, dense) == dense_z
        de.check_stream("one byte", _deflate(gpu_ctx, b"\x7f"), b"\x7f", "gzip", must=["optimal"])
        assert gpu_ctx.bgzf_deflate_device(dense).tobytes() == dense_b
        assert gpu_ctx.bgzf_deflate_device(c.text).tobytes() == b, c.name
        de.check_stream(c.name, b, c.text, "bgzf", de.BGZF_IN)
        assert _deflate(gpu_ctx, b"") == dr.kdeflate_model(b"", [], container="gzip")


def test_two_members_that_share_the_slots(synth, gpu_ctx):
    """smi_scanfastq_pass2_chunk with compress: `passed` and `failed` are deflated one after the other in the same block slots.  A chunk
    whose failed text is much the longer and one the other way round: both members are the model's bytes for the text the uncompressed call gives"""
    wl = synth.make_whitelist(20_000, seed=177)
    used = synth.pick_used(wl, 150, seed=178)
    good = synth.gen_reads(240, used, seed=179, err=0.01)
    g = np.random.default_rng(180)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def junk(i):
        m = int(g.integers(600, 1400))
        return g.choice(acgt, size=m).tobytes().decode(), "".join(chr(33 + int(q)) for q in g.integers(2, 40, size=m))

    def fastq(recs):
        return "".join(f"@read{i} runid=x ch={i % 9}\n{s}\n+\n{q}\n" for i, (s, q) in enumerate(recs)).encode()

    keys = np.sort(used.numpy().astype(np.uint64))
    gpu_ctx.set_barcode_set(keys, mode=0)
    mostly_failed = fastq([synth.materialize(good, i) for i in range(10)] + [junk(i) for i in range(240)])
    mostly_passed = fastq([synth.materialize(good, i) for i in range(240)] + [junk(i) for i in range(8)])
    sizes = []
    for text in (mostly_failed, mostly_passed, mostly_failed):
        p, f, info = gpu_ctx.scanfastq_pass2_chunk(text)
        zp, zf, zinfo = gpu_ctx.scanfastq_pass2_chunk(text, compress=True)
        assert gzip.decompress(bytes(zp)) == bytes(p) and gzip.decompress(bytes(zf)) == bytes(f)
        assert (zinfo["passed_text_bytes"], zinfo["failed_text_bytes"]) == (len(p), len(f))
        de.check_stream("passed", bytes(zp), bytes(p), "gzip")
        de.check_stream("failed", bytes(zf), bytes(f), "gzip")
        sizes.append((len(p), len(f)))
    assert sizes[0] == sizes[2] and 3 * sizes[0][0] < sizes[0][1] and sizes[1][0] > 3 * sizes[1][1] and min(sizes[0] + sizes[1]) > 0, sizes
    assert max(sizes[0]) > 3 * 65536 and max(sizes[1]) > 3 * 65536, sizes          # several blocks in the longer member, one or two in the other
