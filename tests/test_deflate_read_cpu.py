"""The DEFLATE reader and the model of K-DEFLATE (tests/deflateread.py) and the case catalogue (tests/deflateedges.py), proved without the
device before they judge it: the reader against zlib's compressor and against the bit-level writer of tests/deflatecraft.py, the model
against zlib's inflater and the reader (writer <-> reader closure), package-merge against the Huffman cost, the catalogue against what its
families promise, and the comparison itself against four deliberate faults a round trip through an inflater does not notice."""
import zlib

import pytest

import deflatecraft as dc
import deflateedges as de
import deflateread as dr


@pytest.fixture(scope="module")
def small():
    return de.small_cases()


@pytest.fixture(scope="module")
def full():
    return de.full_blocks()


@pytest.mark.parametrize("level,strategy", [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
                                            (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_FIXED), (6, zlib.Z_RLE)])
def test_reader_on_zlibs_own_streams(level, strategy):
    text = dc.fastq_text(90_000, 5)
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    raw = c.compress(text[:40_000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(text[40_000:]) + c.flush()
    blocks = dr.read_deflate(raw)
    assert dr.text_of(blocks) == text and dr.end_byte(blocks) == len(raw) and blocks[-1].final
    kinds = {b.kind for b in blocks}
    assert "stored" in kinds                                                     # (the sync flush in the middle)
    if level == 0 or strategy == zlib.Z_FIXED:
        assert kinds == ({"stored"} if level == 0 else {"fixed", "stored"})
    if strategy == zlib.Z_HUFFMAN_ONLY:
        assert all(b.n_matches == 0 for b in blocks) and "dynamic" in kinds
    if strategy == zlib.Z_DEFAULT_STRATEGY and level:
        assert sum(b.n_matches for b in blocks) > 1000 and "dynamic" in kinds


def test_reader_against_the_writers_blocks():
    """every single-member legal stream of the inflaters' catalogue: the text, and the header as the writer was told to write it"""
    n_dyn = 0
    for c in dc.legal_cases():
        if c.raw is None:
            continue
        got = dr.read_deflate(c.raw)
        assert dr.text_of(got) == c.text and dr.end_byte(got) == len(c.raw), c.name
        assert len(got) == len(c.blocks) and [b.kind for b in got] == [type(b).__name__.lower() for b in c.blocks], c.name
        for g, w in zip(got, c.blocks):
            assert g.final == bool(w.final)
            if g.kind == "dynamic":
                n_dyn += 1
                assert (g.ll_lens, g.d_lens, g.cl_symbols) == (w.ll_lens, w.d_lens, w.cl_symbols), c.name
                assert (g.hlit, g.hdist, g.hclen) == (len(w.ll_lens), len(w.d_lens), w.hclen) and g.cl_lens[:] == [
                    w.cl_lens[s] if dc.CL_ORDER.index(s) < w.hclen else 0 for s in range(19)], c.name
                assert g.eob_bit == w.eob_at, c.name
    assert n_dyn > 100


def test_reader_refuses_the_illegal_streams():
    n = 0
    for c in dc.illegal_cases():
        if c.raw is not None:
            n += 1
            with pytest.raises(dr.DeflateError):
                dr.read_deflate(c.raw)
                pytest.fail(c.name)
    assert n >= 18
    raw = de.rendered(b"GATTACA" * 900, "raw")             # measured, not decoded: the end-of-block code must stand where the text ends
    dr.read_deflate(raw, [b"GATTACA" * 900])
    for wrong in (b"GATTACA" * 899 + b"GATTAC", b"GATTACA" * 900 + b"G", b"GATTACA" * 899 + b"GATTACN"):
        with pytest.raises(dr.DeflateError):
            dr.read_deflate(raw, [wrong])


def test_tokens_of_the_header():
    def lens(used):
        return [1 if s in used or s == 256 else 0 for s in range(257)]

    t = dr.kdeflate_tokens
    assert t(lens(range(256))) == [(1, 0)] * 257 + [(0, 0)]
    assert t(lens([])) == [(18, 127), (18, 256 - 138 - 11), (1, 0), (0, 0)]                       # 255 is never followed by a run into 256
    assert t(lens([138])) == [(18, 127), (1, 0), (18, 117 - 11), (1, 0), (0, 0)]
    assert t(lens([139])) == [(18, 127), (0, 0), (1, 0), (18, 116 - 11), (1, 0), (0, 0)]
    assert t(lens([140]))[:4] == [(18, 127), (0, 0), (0, 0), (1, 0)]
    assert t(lens([141]))[:3] == [(18, 127), (17, 0), (1, 0)] and t(lens([148]))[:3] == [(18, 127), (17, 7), (1, 0)]
    assert t(lens([149]))[:3] == [(18, 127), (18, 0), (1, 0)] and t(lens([137]))[:2] == [(18, 126), (1, 0)]
    assert t(lens([10]))[:2] == [(17, 7), (1, 0)] and t(lens([11]))[:2] == [(18, 0), (1, 0)] and t(lens([2]))[:3] == [(0, 0), (0, 0), (1, 0)]
    assert t(lens(range(255)))[-4:] == [(1, 0), (0, 0), (1, 0), (0, 0)]                           # the zero at 255 and the distance length: two singles
    # the zeros cut as the writer's serial greedy coder cuts them over the 256 literal positions (that one also repeats lengths: symbol 16)
    for c in de.long_run_cases() + de.gap_cases():
        h = de.hist257(c.text)
        zeros = [k for k in dc.run_symbols([1 if h[s] else 0 for s in range(256)]) if k[0] in (0, 17, 18)]
        assert [k for k in t(lens({s for s in range(256) if h[s]}))[:-2] if k[0] != 1] == zeros, c.name


def _closure(name, text, container, block_in):
    pieces = [text[at:at + block_in] for at in range(0, len(text), block_in)]
    lens = [dc.huff_lengths(de.hist257(p), 15) for p in pieces]
    out = dr.kdeflate_model(text, lens, block_in, container)
    back = zlib.decompress(out, -15) if container == "raw" else dc.gunzip_reference(out)[0]
    assert back == text, name
    at = 0
    for raw, _, _ in dr.payloads(out, container):
        k = 1 if container == "bgzf" else len(pieces)
        blocks = dr.read_deflate(raw, [t for p in pieces[at:at + k] for t in (p if len(p) > dr.SKIP_ABOVE else None, None)])
        assert dr.end_byte(blocks) == len(raw) and len(blocks) == 2 * k + 1, name
        for j in range(k):
            b = blocks[2 * j]
            assert b.ll_lens == lens[at + j] and b.cl_symbols == dr.kdeflate_tokens(lens[at + j]) and b.text == pieces[at + j], (name, j)
        at += k
    assert at == len(pieces)
    return out


def test_model_inflates_and_reads_back_small(small):
    for c in small:
        for container in ("gzip", "raw"):
            _closure(c.name, c.text, container, 65536)
    for c in de.long_run_cases():
        _closure(c.name, c.text, "bgzf", de.BGZF_IN)
    assert dr.kdeflate_model(b"", [], 65536, "gzip") == dc.gzip_member(b"\x03\x00", b"") and dr.kdeflate_model(b"", [], de.BGZF_IN, "bgzf") == dr.BGZF_EOF


def test_model_inflates_and_reads_back_full_blocks_and_seams(full):
    text = b"".join(c.text for c in full)
    assert all(len(c.text) == 65536 for c in full[:-1]) and 20 <= len(full) <= 26
    out = _closure("full", text, "gzip", 65536)
    assert dr.kdeflate_model(text, [dc.huff_lengths(de.hist257(c.text), 15) for c in full], 65536, "raw") == out[10:-8]
    for n in de.SEAM_SIZES:
        _closure(f"seam/{n}", de.seam_text(n), "raw", 65536)
    for n in de.BGZF_SIZES:
        _closure(f"bgzf/{n}", de.seam_text(n), "bgzf", de.BGZF_IN)


def test_package_merge(small, full):
    cases = small[::8] + [c for c in small if c.name.startswith(("ties/", "one_byte/"))][::3] + full
    n_limited = 0
    for c in cases:
        h = de.hist257(c.text[:65536])
        pm = dr.package_merge(h, 15)
        assert all((n != 0) == (f != 0) for n, f in zip(pm, h)) and dr.kraft(pm) == 1 << 15 and max(pm) <= 15, c.name
        cost, free = dr.cost_of(h, pm), dr.optimal_cost(h)
        assert free <= cost <= dr.cost_of(h, dc.huff_lengths(h, 15)), c.name
        deep = max(dc.huff_lengths(h, 1 << 30))
        if deep <= 15:
            assert cost == free, c.name
        else:
            n_limited += 1
    assert n_limited >= 4
    h = [1, 1, 2, 3, 5, 8, 13, 21]                  # depth 7 unlimited; limits from 3 (the least for 8 symbols) upwards
    costs = [dr.cost_of(h, dr.package_merge(h, limit)) for limit in range(3, 9)]
    assert costs[0] == 3 * sum(h) and costs == sorted(costs, reverse=True) and costs[-2:] == [dr.optimal_cost(h)] * 2
    assert all(dr.kraft(dr.package_merge(h, limit), limit) == 1 << limit for limit in range(3, 9))


def test_catalogue_is_what_its_families_promise(small, full):
    names = [c.name for c in small + full]
    assert len(set(names)) == len(names) and len(de.gap_cases()) == 128 and len(de.tie_cases()) == 200
    for c in small:
        assert 1 <= len(c.text) <= de.SMALL and c.must == "optimal", c.name          # 2049 < F(18): nothing to flatten
    gaps = {(c.name, tuple(s for s in range(256) if not de.hist257(c.text)[s])) for c in de.gap_cases()}
    assert ("gap/193+63", tuple(range(193, 256))) in gaps and ("gap/0+1", (0,)) in gaps and ("gap/63+2", (63, 64)) in gaps
    for c in de.tie_cases():
        assert 1 <= sum(1 for f in de.hist257(c.text)[:256] if f) <= 15, c.name
    for c in full:
        h = de.hist257(c.text)
        lits = [f for f in h[:256] if f]
        rendered, halvings = dr.kdeflate_lengths(h)
        if c.must == "optimal" and len(c.text) <= de.SMALL:
            continue
        if c.must == "optimal":
            assert len(lits) <= 15 or max(lits) < 2 * min(lits), c.name
            assert halvings == 0 and max(dc.huff_lengths(h, 1 << 30)) <= (15 if len(lits) <= 15 else 11) and max(rendered) <= (15 if len(lits) <= 15 else 11), c.name
        if c.must == "flat":
            # no Huffman code of it is 15 deep or less: the length-limited optimum costs more
            assert dr.cost_of(h, dr.package_merge(h, 15)) > dr.optimal_cost(h) and halvings >= 1, c.name
    assert sum(c.must == "optimal" for c in full[:-1]) >= 16 and sum(c.must == "flat" for c in full) == 4


def test_the_rendering_passes_the_comparison(small, full):
    """the comparison the device's output is put through, on the model's bytes for the lengths of the rule K-DEFLATE states: it passes, and the
    figures of the flattened blocks are inside their bounds"""
    for c in small:
        de.check_stream(c.name, de.rendered(c.text, "gzip"), c.text, "gzip", must=[c.must])
    for c in de.long_run_cases():
        de.check_stream(c.name, de.rendered(c.text, "bgzf", de.BGZF_IN), c.text, "bgzf", de.BGZF_IN, [c.must])
    text = b"".join(c.text for c in full)
    figs = de.check_stream("full", de.rendered(text, "raw"), text, "raw", must=[c.must for c in full])
    flat = [f for f in figs if f["must"] == "flat"]
    assert len(flat) == 4 and all(f["optimum"] <= f["cost"] <= f["bound"] for f in flat)
    for n in (0, 1, 65473, 65536 + 64):
        de.check_stream(f"seam/{n}", de.rendered(de.seam_text(n), "gzip"), de.seam_text(n), "gzip")
    for n in (61441, 122880):
        de.check_stream(f"bgzf/{n}", de.rendered(de.seam_text(n), "bgzf", de.BGZF_IN), de.seam_text(n), "bgzf", de.BGZF_IN)


# ---- sensitivity: four faults zlib inflates without a word ---------------------------------------------------------------------------
def _case(cases, name):
    return next(c for c in cases if c.name == name)


def _fails(name, out, text, must, word):
    assert dc.gunzip_reference(out)[0] == text, (name, "the faulty stream must still be a legal member of the text")
    with pytest.raises(AssertionError) as e:
        de.check_stream(name, out, text, "gzip", must=[must])
    assert word in str(e.value), (name, str(e.value)[:300])


def test_a_tied_pair_of_lengths_swapped_is_noticed(small):
    c = _case(small, "ties/3_4lit")
    h = de.hist257(c.text)
    lens, _ = dr.kdeflate_lengths(h)
    a, b = next((a, b) for a in range(257) for b in range(a + 1, 257) if h[a] and h[a] == h[b] and lens[a] != lens[b])
    lens[a], lens[b] = lens[b], lens[a]
    assert dr.cost_of(h, lens) == dr.optimal_cost(h)                   # as cheap as before: only the order tells
    _fails(c.name, de.rendered(c.text, lens=[lens]), c.text, c.must, "lengths must not grow")


def test_a_run_of_138_cut_as_137_and_1_is_noticed(small):
    c = _case(small, "one_byte/138")

    def cut(lens):
        t = dr.kdeflate_tokens(lens)
        assert t[0] == (18, 127)
        return [(18, 126), (0, 0)] + t[1:]

    _fails(c.name, de.rendered(c.text, tokens=cut), c.text, c.must, "header tokens")


def test_a_length_raised_and_another_lowered_is_noticed(small):
    c = _case(small, "gap/64+3")
    h = de.hist257(c.text)
    lens, _ = dr.kdeflate_lengths(h)
    a, b = next((a, b) for a in range(257) for b in range(257) if lens[a] and lens[b] == lens[a] + 1 and h[a] > h[b] + 1)
    lens[a] += 1
    lens[b] -= 1
    assert dr.kraft(lens) == 1 << 15
    _fails(c.name, de.rendered(c.text, lens=[lens]), c.text, c.must, "lengths must not grow")
    # a code flattened when it need not be (the best one that is a bit shallower) is complete and in order: only its cost tells
    c = _case(small, "ties/2_3lit")
    h = de.hist257(c.text)
    lens, _ = dr.kdeflate_lengths(h)
    flat = dr.package_merge(h, max(lens) - 1)
    along = sorted((n for n in flat if n), reverse=True)
    for (_, s), n in zip(sorted((f, s) for s, f in enumerate(h) if f), along):
        flat[s] = n
    assert dr.kraft(flat) == 1 << 15 and dr.cost_of(h, flat) > dr.optimal_cost(h)
    _fails(c.name, de.rendered(c.text, lens=[flat]), c.text, c.must, "not a minimum-redundancy code")


def test_a_padding_bit_set_is_noticed(small):
    c = _case(small, "gap/31+1")
    out = bytearray(de.rendered(c.text))
    sync = dr.read_deflate(bytes(out[10:-8]))[1]
    assert sync.kind == "stored" and sync.pad_bits >= 1
    at = sync.start_bit + 3                       # the first bit behind BFINAL and BTYPE
    out[10 + (at >> 3)] |= 1 << (at & 7)
    _fails(c.name, bytes(out), c.text, c.must, "padding bits must be zero")
