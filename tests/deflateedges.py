"""The edge cases of K-DEFLATE (smi_deflate.hip) and the comparison its output is put through, shared by the tests that run without the
device (which prove the reader, the model and the catalogue) and those that run on it.  Imports nothing of the project.

A case is a byte string made from a prescribed histogram and shuffled with a fixed seed, so that which literals are used, how often and
where the zero runs of the header lie is exactly what the case says.

  zero runs    all bytes used but one gap [s, s + r): a run of every critical length at every seam of the header's token placement (lane
               63/64, 127/128, 191/192 = the wave scan plus wave sums; 31/32 .. = the words of the non-zero bit map); one byte used (runs
               of 1 .. 255 from position 0 and up to 255), two, every second, every third, all
  ties         1 .. 15 distinct literals, frequencies from a short list full of ties
  full blocks  64 KiB each: those that must come out optimal (at most 15 literals; many literals within a factor of two), those that must
               be flattened to 15 bits (Fibonacci and kin)
  seams        sizes around the runs of 64 bytes, around 16384 / 32768 / 49152 (where the thread that owns a run starts over) and the block
               size, from input pointers of every alignment

`check_stream` is the comparison: zlib inflates the output to the text; the reader accounts for every bit and finds the structure K-DEFLATE
is meant to write; the output EQUALS the model's bytes for the code lengths the reader found; those lengths are a complete code of at most
15 bits, ordered as (frequency, symbol) orders the literals, and as cheap as the case demands."""
import zlib

import numpy as np

import deflatecraft as dc
import deflateread as dr

FIB_18 = 2584        # a Huffman code is L deep only if the weights sum to F(L + 2) or more (F(1) = F(2) = 1): 16 deep needs 2584
SMALL = 2048         # bytes of a small case at most: with the end-of-block code 2049 < 2584, so no code of such a text is 16 deep

GAP_STARTS = (0, 1, 30, 31, 32, 62, 63, 64, 65, 126, 127, 128, 190, 191, 192, 193)
GAP_RUNS = (1, 2, 3, 4, 10, 11, 12, 64)
ONE_BYTE = (0, 1, 2, 3, 10, 11, 137, 138, 139, 140, 141, 148, 149, 254, 255)
SEAM_SIZES = (63, 64, 65, 127, 128, 129, 16383, 16384, 16385, 16447, 16448, 32767, 32768, 32769, 49151, 49152, 49153, 65471, 65472, 65473,
              65536 + 63, 65536 + 64, 65536 + 65)
SEAM_OFFSETS = (0, 1, 4, 8, 15)
BGZF_IN = 61440
BGZF_SIZES = (61439, 61440, 61441, 61440 + 63, 61440 + 64, 61440 + 65, 122879, 122880, 122881)


class Edge:
    """name; text; must: "optimal" (the code costs what a Huffman code costs), "flat" (it was flattened to 15 bits: within the bound of
    check_lengths of the length-limited optimum) or None (no demand beyond a complete, ordered code)"""

    def __init__(self, name, text, must=None):
        self.name, self.text, self.must = name, bytes(text), must

    def __repr__(self):
        return f"Edge({self.name})"


def hist257(text):
    """the histogram K-DEFLATE codes a block by: the 256 literals and one end-of-block"""
    return [int(v) for v in np.bincount(np.frombuffer(text, dtype=np.uint8), minlength=256)] + [1]


def text_of_hist(hist, seed):
    a = np.repeat(np.arange(256, dtype=np.uint8), np.asarray(hist[:256], dtype=np.int64))
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def _fit(freqs, cap):
    """the same frequencies with the largest ones cut until they sum to `cap` at most"""
    freqs = [int(f) for f in freqs]
    while sum(freqs) > cap:
        k = max(range(len(freqs)), key=lambda i: freqs[i])
        freqs[k] = max(1, freqs[k] // 2)
    return freqs


def _from_used(name, used, seed, must="optimal"):
    g = np.random.default_rng(seed)
    f = _fit(1 + np.minimum(g.geometric(0.2, size=len(used)) - 1, 60), SMALL)
    hist = [0] * 256
    for s, v in zip(used, f):
        hist[s] = v
    return Edge(name, text_of_hist(hist, seed + 1), must)


def gap_cases():
    """all bytes but [s, s + r)"""
    out = []
    for s in GAP_STARTS:
        for r in GAP_RUNS:
            e = min(256, s + r)
            out.append(_from_used(f"gap/{s}+{e - s}", [b for b in range(256) if not s <= b < e], 1000 * s + r))
    return out


def long_run_cases():
    out = [Edge(f"one_byte/{b}", bytes([b]) * (100 + b), "optimal") for b in ONE_BYTE]
    out.append(_from_used("two_bytes/0_255", [0, 255], 5))
    out.append(_from_used("every_second", list(range(0, 256, 2)), 6))
    out.append(_from_used("every_second_from_1", list(range(1, 256, 2)), 7))
    out.append(_from_used("every_third", list(range(0, 256, 3)), 8))
    out.append(_from_used("all_256", list(range(256)), 9))
    return out


def tie_cases(n=200):
    draw = [1, 1, 1, 2, 2, 3, 4, 8, 16, 32, 64, 128, 256, 512]
    out = []
    for k in range(n):
        g = np.random.default_rng(7000 + k)
        n_lit = 1 + k % 15
        syms = sorted(int(s) for s in g.choice(256, size=n_lit, replace=False))
        f = _fit(g.choice(draw, size=n_lit), SMALL)
        hist = [0] * 256
        for s, v in zip(syms, f):
            hist[s] = v
        out.append(Edge(f"ties/{k}_{n_lit}lit", text_of_hist(hist, 8000 + k), "optimal"))
    return out


def small_cases():
    return gap_cases() + long_run_cases() + tie_cases()


def _block(name, freqs, syms, seed, must):
    assert sum(freqs) == 65536 and len(freqs) == len(syms) and min(freqs) >= 1, (name, sum(freqs))
    hist = [0] * 256
    for s, v in zip(syms, freqs):
        hist[s] = int(v)
    return Edge(name, text_of_hist(hist, seed), must)


def _to_block(freqs, at=-1):
    """the frequencies with the difference to 65536 put on entry `at`"""
    freqs = [int(f) for f in freqs]
    freqs[at] += 65536 - sum(freqs)
    return freqs


def optimal_blocks():
    """full blocks whose code must cost what a Huffman code costs.  (a) at most 15 literals: with the end-of-block code 16 symbols, no code
    of which is deeper than 15; (b) many literals whose frequencies lie within a factor of two of each other: once the end-of-block code
    (weight 1) has joined the lightest literal, every round of pairings at least doubles the lightest weight and n symbols within a factor
    of two end at most ceil(log2 n) + 1 deep, 11 with the end-of-block pair for 256 literals -- whatever the order among equals"""
    letters = list(b"ACGTN\n@+!5?IFab")          # 15
    g = np.random.default_rng(65536)
    out = [
        _block("opt/a_one_literal", [65536], [71], 1, "optimal"),
        _block("opt/a_two_equal", [32768, 32768], [0, 255], 2, "optimal"),
        _block("opt/a_1_1_rest", [1, 1, 65534], [10, 65, 200], 3, "optimal"),
        _block("opt/a_eight_equal", [8192] * 8, letters[:8], 4, "optimal"),
        _block("opt/a_fifteen_equal", _to_block([4369] * 15), letters, 5, "optimal"),
        _block("opt/a_powers_of_two_15", [4, 4] + [1 << k for k in range(3, 16)], letters, 6, "optimal"),
        _block("opt/a_fibonacci_15", _to_block([1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610]), letters, 7, "optimal"),
        _block("opt/a_ones_and_one_heavy", _to_block([1] * 14 + [1]), letters, 8, "optimal"),
        _block("opt/a_pairs_of_ties", _to_block([3, 3, 6, 6, 12, 12, 24, 24, 48, 48, 96, 96, 192, 192, 1]), letters, 9, "optimal"),
    ]
    for k in range(3):
        f = g.integers(1, 2000, size=15) ** int(1 + k)
        out.append(_block(f"opt/a_random_{k}", _to_block(np.maximum(1, f * 60000 // f.sum())), sorted(int(s) for s in g.choice(256, 15, replace=False)),
                          10 + k, "optimal"))
    out.append(_block("opt/b_256_equal", [256] * 256, list(range(256)), 20, "optimal"))
    for k, n in enumerate((256, 100, 61, 40)):
        base = 65536 // n * 2 // 3                                   # frequencies in [base, 2 * base)
        f = base + g.integers(0, base, size=n)
        f = np.minimum(np.maximum(base, f * (65536 - n) // f.sum()), 2 * base - 1)
        f = [int(v) for v in f]
        at = 0
        while sum(f) != 65536:                                       # the rest a unit at a time, inside the factor of two
            step = 1 if sum(f) < 65536 else -1
            if base <= f[at % n] + step < 2 * base:
                f[at % n] += step
            at += 1
        assert max(f) < 2 * min(f)
        out.append(_block(f"opt/b_{n}_within_2x", f, sorted(int(s) for s in g.choice(256, n, replace=False)), 30 + k, "optimal"))
    return out


def flat_blocks():
    """full blocks no Huffman code of which is 15 deep or less (the tests without the device show it: the length-limited optimum costs more
    than the Huffman code)"""
    fib = [1, 2]          # the end-of-block code is the other 1
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    geo = [max(1, round(65536 * 0.45 * 0.55 ** k)) for k in range(40)]
    return [
        _block("flat/fibonacci_22", _to_block(fib), list(range(65, 86)), 40, "flat"),
        _block("flat/fibonacci_20_plus_40_flat", _to_block(fib[:19] + [1195] * 40), list(range(33, 92)), 41, "flat"),
        _block("flat/powers_of_two_17", [1, 1] + [1 << k for k in range(1, 16)], list(range(97, 114)), 42, "flat"),
        _block("flat/geometric_0.55_40", _to_block(geo, 0), list(range(48, 88)), 43, "flat"),
    ]


def full_blocks():
    """the blocks of the one batched member: every block but the last is exactly 64 KiB"""
    out = optimal_blocks() + flat_blocks()
    out.append(Edge("full/fastq", dc.fastq_text(70_000, 21)[:65536]))
    out.append(Edge("full/short_last", dc.fastq_text(3000, 22)[:1500], "optimal"))
    return out


_SEAM = []


def seam_text(n):
    """n bytes of FASTQ-like text"""
    if not _SEAM:
        _SEAM.append(dc.fastq_text(140_000, 33))
    return _SEAM[0][:n]


# ---- the comparison -------------------------------------------------------------------------------------------------------------------
def halvings_bound(hist):
    """the smallest k for which the frequencies halved k times (rounded up) sum to less than F(18) = 2584: after that many halvings no
    Huffman code of them is 16 deep, so K-DEFLATE's loop "halve while a length exceeds 15" has ended by then"""
    k = 0
    while sum(-(-f >> k) for f in hist if f) >= FIB_18:
        k += 1
    return k


def check_lengths(name, hist, lens, must):
    """the code lengths of one block against its histogram (257 entries each) -> dict of the figures"""
    assert all((n != 0) == (f != 0) for n, f in zip(lens, hist)), (name, "a code exactly where the symbol occurs")
    assert max(lens) <= 15 and dr.kraft(lens) == 1 << 15, (name, "a complete code of at most 15 bits", max(lens), dr.kraft(lens))
    order = sorted((f, s) for s, f in enumerate(hist) if f)
    along = [lens[s] for _, s in order]
    assert all(a >= b for a, b in zip(along, along[1:])), (name, "lengths must not grow along (frequency, symbol)", order, along)
    cost = dr.cost_of(hist, lens)
    fig = dict(name=name, cost=cost, must=must)
    if must == "optimal":
        best = dr.optimal_cost(hist)
        assert cost == best, (name, "not a minimum-redundancy code", cost, best)
    elif must == "flat":
        # The flattened code is a Huffman code of g = ceil(f / 2^k) for some k <= K, so it costs no more under g than the package-merge
        # code does, and f <= 2^k g < f + 2^k:  cost_f(dev) <= 2^k cost_g(dev) <= 2^k cost_g(pm) < cost_f(pm) + 2^k sum(pm lengths)
        pm = dr.package_merge(hist, 15)
        best, k = dr.cost_of(hist, pm), halvings_bound(hist)
        bound = best + (1 << k) * sum(pm)
        fig.update(optimum=best, bound=bound, halvings_at_most=k, excess=cost - best)
        print(f"{name}: cost {cost}, package-merge optimum {best}, bound {bound} (K = {k}), excess {cost - best}")
        assert cost >= best, (name, "cheaper than the length-limited optimum: the reference is wrong", cost, best)
        assert cost <= bound, (name, "flattened further than the halving rule can", cost, best, bound)
    return fig


_MODELS = {}


def _model(text, lens, block_in, container):
    key = (text, tuple(tuple(v) for v in lens), block_in, "bgzf" if container == "bgzf" else "gzip")
    if key not in _MODELS:
        if len(_MODELS) >= 4:
            _MODELS.clear()
        _MODELS[key] = dr.kdeflate_model(text, lens, block_in, key[3])
    m = _MODELS[key]
    return m[10:-8] if container == "raw" else m          # (a member is its header, the raw stream and its trailer)


def check_stream(name, out, text, container="gzip", block_in=65536, must=None):
    """`out` is what K-DEFLATE must write for `text`; must: per block, see Edge -> the figures of check_lengths per block"""
    out, text = bytes(out), bytes(text)
    pieces = [text[at:at + block_in] for at in range(0, len(text), block_in)]
    must = list(must) if must is not None else [None] * len(pieces)
    assert len(must) == len(pieces)
    # 1. an independent inflater
    if container == "raw":
        d = zlib.decompressobj(-15)
        assert d.decompress(out) == text and d.eof and not d.unused_data, (name, "zlib does not inflate it to the text")
    else:
        back, n = dc.gunzip_reference(out)
        assert back == text and n == (len(pieces) + 1 if container == "bgzf" else 1), (name, "zlib does not inflate it to the text", n)
    # 2. every bit accounted for, the structure
    streams = dr.payloads(out, container)
    groups = [[p] for p in pieces] if container == "bgzf" else [pieces]
    assert len(streams) == len(groups), (name, len(streams), len(groups))
    lens_all = []
    for (raw, crc, isize), group in zip(streams, groups):
        texts = [t for p in group for t in (p if len(p) > dr.SKIP_ABOVE else None, None)] + [None]
        blocks = dr.read_deflate(raw, texts)
        assert dr.end_byte(blocks) == len(raw), (name, "bytes behind the last block", dr.end_byte(blocks), len(raw))
        assert [b.kind for b in blocks] == ["dynamic", "stored"] * len(group) + ["fixed"], (name, blocks)
        assert [b.final for b in blocks] == [False] * (2 * len(group)) + [True], (name, blocks)
        for k, p in enumerate(group):
            dyn, sync = blocks[2 * k], blocks[2 * k + 1]
            assert (dyn.hlit, dyn.hdist, dyn.hclen) == (257, 1, 19) and dyn.cl_lens == dr.KD_CL_LENS and dyn.d_lens == [0], (name, k, vars(dyn))
            assert dyn.text == p and dyn.n_matches == 0, (name, k, "the block's text")
            assert dyn.cl_symbols == dr.kdeflate_tokens(dyn.ll_lens), (name, k, "header tokens", dyn.cl_symbols, dr.kdeflate_tokens(dyn.ll_lens))
            assert sync.text == b"" and sync.pad_value == 0, (name, k, "padding bits must be zero", sync.pad_bits, sync.pad_value)
            lens_all.append(dyn.ll_lens)
        last = blocks[-1]
        assert last.text == b"" and last.tail_value == 0 and raw[-2:] == b"\x03\x00", (name, "the last block", raw[-2:])
        if crc is not None:
            t = b"".join(group)
            assert (crc, isize) == (zlib.crc32(t), len(t) & 0xFFFFFFFF), (name, "trailer", crc, isize)
    if container == "bgzf":
        assert all(len(m) <= 65536 for m in dc.bgzf_blocks(out)), (name, "a BGZF block above 64 KiB")
    # 3. the model's bytes
    model = _model(text, lens_all, block_in, container)
    if out != model:
        k = next((j for j in range(min(len(out), len(model))) if out[j] != model[j]), min(len(out), len(model)))
        raise AssertionError((name, container, "differs from the model", len(out), len(model), "first at byte", k, out[max(0, k - 8):k + 8].hex(),
                              model[max(0, k - 8):k + 8].hex()))
    # 4. the code lengths
    return [check_lengths(f"{name}[{k}]", hist257(p), lens, m) for k, (p, lens, m) in enumerate(zip(pieces, lens_all, must))]


def rendered(text, container="gzip", block_in=65536, tokens=dr.kdeflate_tokens, lens=None):
    """a stand-in for the device where there is none: the model's bytes for the lengths of dr.kdeflate_lengths (or `lens`)"""
    text = bytes(text)
    if lens is None:
        lens = [dr.kdeflate_lengths(hist257(text[at:at + block_in]))[0] for at in range(0, len(text), block_in)]
    return dr.kdeflate_model(text, lens, block_in, container, tokens)
