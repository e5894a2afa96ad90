"""A DEFLATE reader for tests and a byte-exact model of K-DEFLATE (smi_deflate.hip), pure Python plus numpy and independent of the project.

`read_deflate` walks a raw RFC 1951 stream bit by bit and returns one record per block: what the header SAYS (the count fields, the lengths
of the code-length code, the code-length symbol sequence as written, both arrays of code lengths), where every part of the block lies, and
the padding bits that were skipped.  zlib's inflater says whether a stream is legal and what it means; this reader says which stream it is.

`kdeflate_model` writes, with the writer of tests/deflatecraft.py, the stream K-DEFLATE is meant to write for a text: one literal-only dynamic
block per 64 KiB (61,440 bytes in BGZF), each followed by the empty stored block, the empty fixed block at the end, in a gzip member, bare, or
as BGZF.  The code lengths of every block are the model's only input besides the text; canonical codes, bit order, the header's fields and
its zero-run tokens, the padding and the trailers are the model's own.

`optimal_cost`, `package_merge` and `kdeflate_lengths` are what the code lengths are held against."""
import heapq
import zlib

import numpy as np

import deflatecraft as dc

SKIP_ABOVE = 4096          # texts up to this size are decoded symbol by symbol, longer literal-only blocks are measured (see read_deflate)

# the code-length code K-DEFLATE always writes: 4 bits for {0, 2..12, 17, 18}, 5 for {1, 13, 14, 15}, none for 16; all 19 lengths are sent
KD_CL_LENS = [0 if s == 16 else 5 if s in (1, 13, 14, 15) else 4 for s in range(19)]
BGZF_EOF = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


class DeflateError(ValueError):
    """the stream is not DEFLATE (or ends too early)"""


class Block:
    """one block of a stream.  kind: "stored" / "fixed" / "dynamic"; final; start_bit .. end_bit (the padding behind the last block not
    included); pad_bits / pad_value: the bits a stored block skips in front of LEN; tail_bits / tail_value (last block only): the bits
    between the end of the stream and the end of its byte; text: the bytes the block stands for; n_matches.
    dynamic: hlit, hdist, hclen (the counts, not the fields: 257.., 1.., 4..), cl_lens (19, by symbol), cl_symbols [(symbol, extra value)],
    ll_lens, d_lens, body_bit (the first code), eob_bit (the end-of-block code); decoded: False where the body was measured, not decoded"""

    def __init__(self, kind, final, start_bit):
        self.kind, self.final, self.start_bit = kind, final, start_bit
        self.end_bit = None
        self.pad_bits = self.pad_value = self.tail_bits = self.tail_value = 0
        self.text, self.n_matches, self.decoded = b"", 0, True

    def __repr__(self):
        return f"Block({self.kind}, bits {self.start_bit}..{self.end_bit}, {len(self.text)} bytes{', final' if self.final else ''})"


class _Bits:
    def __init__(self, raw):
        self.raw, self.pos, self.end = bytes(raw), 0, 8 * len(raw)

    def take(self, k):
        if self.pos + k > self.end:
            raise DeflateError("truncated stream")
        v = self.peek(k)
        self.pos += k
        return v

    def peek(self, k):
        """the next k <= 16 bits, zeros behind the end of the stream"""
        i = self.pos >> 3
        return (int.from_bytes(self.raw[i:i + 4], "little") >> (self.pos & 7)) & ((1 << k) - 1)


def _decoder(lens, what, lengths_code=False):
    """code lengths -> (table indexed by the next `width` bits as they lie in the stream, width); an entry is (symbol, length) or None.
    Refused: an over-subscribed code; an incomplete one unless it is a single code of one bit (what inflate accepts) -- never for the
    code-length code"""
    width = max(lens) if lens else 0
    if width == 0:
        return [None], 0
    if width > 15:
        raise DeflateError(f"{what}: a code of {width} bits")
    left = 1 << width
    for n in lens:
        if n:
            left -= 1 << (width - n)
    if left < 0:
        raise DeflateError(f"{what}: over-subscribed code")
    if left > 0 and (lengths_code or width != 1):
        raise DeflateError(f"{what}: incomplete code")
    table = [None] * (1 << width)
    for s, (n, c) in enumerate(zip(lens, dc.canonical(list(lens)))):
        if n:
            table[c::1 << n] = [(s, n)] * (1 << (width - n))
    return table, width


def _symbol(bits, dec, what):
    table, width = dec
    e = table[bits.peek(width)] if width else None
    if e is None:
        raise DeflateError(f"{what}: invalid code")
    if bits.pos + e[1] > bits.end:
        raise DeflateError("truncated stream")
    bits.pos += e[1]
    return e[0]


_FIXED = None


def _fixed_decoders():
    global _FIXED
    if _FIXED is None:
        _FIXED = _decoder(dc.FIXED_LL, "fixed literal/length code"), _decoder(dc.FIXED_D, "fixed distance code")
    return _FIXED


def _body(bits, blk, ll, d, out):
    """the codes of a block up to its end-of-block code, expanded behind `out`"""
    start = len(out)
    while True:
        at = bits.pos
        s = _symbol(bits, ll, "literal/length")
        if s < 256:
            out.append(s)
        elif s == 256:
            blk.eob_bit = at
            break
        else:
            if s > 285:
                raise DeflateError(f"literal/length symbol {s}")
            length = dc.LEN_BASE[s - 257] + bits.take(dc.LEN_EXTRA[s - 257])
            t = _symbol(bits, d, "distance")
            if t > 29:
                raise DeflateError(f"distance symbol {t}")
            dist = dc.DIST_BASE[t] + bits.take(dc.DIST_EXTRA[t])
            if dist > len(out):
                raise DeflateError("distance beyond the start of the text")
            for _ in range(length):
                out.append(out[-dist])
            blk.n_matches += 1
    blk.text = bytes(out[start:])


def _dynamic_header(bits, blk):
    blk.hlit, blk.hdist, blk.hclen = 257 + bits.take(5), 1 + bits.take(5), 4 + bits.take(4)
    if blk.hlit > 286 or blk.hdist > 30:
        raise DeflateError(f"HLIT {blk.hlit} / HDIST {blk.hdist}")
    blk.cl_lens = [0] * 19
    for k in range(blk.hclen):
        blk.cl_lens[dc.CL_ORDER[k]] = bits.take(3)
    cl = _decoder(blk.cl_lens, "code-length code", lengths_code=True)
    lens, blk.cl_symbols, want = [], [], blk.hlit + blk.hdist
    while len(lens) < want:
        s = _symbol(bits, cl, "code length")
        if s < 16:
            blk.cl_symbols.append((s, 0))
            lens.append(s)
            continue
        x = bits.take({16: 2, 17: 3, 18: 7}[s])
        blk.cl_symbols.append((s, x))
        if s == 16 and not lens:
            raise DeflateError("repeat without a length in front of it")
        n = x + (3 if s < 18 else 11)
        if len(lens) + n > want:
            raise DeflateError("repeat past the last code length")
        lens += [lens[-1] if s == 16 else 0] * n
    blk.ll_lens, blk.d_lens = lens[:blk.hlit], lens[blk.hlit:]
    if not blk.ll_lens[256]:
        raise DeflateError("no end-of-block code")
    blk.body_bit = bits.pos


def read_deflate(raw, texts=None):
    """-> [Block] of the raw DEFLATE stream at the start of `raw`; DeflateError for anything inflate refuses.  texts: per block, None (decode
    it) or the text of a literal-only dynamic block, whose body is then not decoded but measured: its codes take sum(hist[s] * ll_lens[s])
    bits, every byte value of the text must have a code, and the end-of-block code must stand exactly behind them (the caller compares
    the bytes of the stream with a model's; this only finds the block's end)"""
    bits, out, blocks = _Bits(raw), bytearray(), []
    while True:
        final, kind = bits.take(1), bits.take(2)
        blk = Block(("stored", "fixed", "dynamic", "reserved")[kind], bool(final), bits.pos - 3)
        given = texts[len(blocks)] if texts is not None and len(blocks) < len(texts) else None
        if kind == 3:
            raise DeflateError("block type 3")
        if kind == 0:
            blk.pad_bits = -bits.pos & 7
            blk.pad_value = bits.take(blk.pad_bits)
            n, nn = bits.take(16), bits.take(16)
            if n ^ nn != 0xFFFF:
                raise DeflateError("stored block: LEN and NLEN do not fit")
            if bits.pos + 8 * n > bits.end:
                raise DeflateError("truncated stream")
            blk.text = bits.raw[bits.pos >> 3:(bits.pos >> 3) + n]
            out += blk.text
            bits.pos += 8 * n
        else:
            if kind == 1:
                ll, d = _fixed_decoders()
            else:
                _dynamic_header(bits, blk)
                ll = d = None
            if given is not None and kind == 2:
                hist = np.bincount(np.frombuffer(given, dtype=np.uint8), minlength=256)
                lens = np.asarray(blk.ll_lens[:256])
                if ((hist > 0) & (lens == 0)).any():
                    raise DeflateError("a byte of the given text has no code")
                bits.pos += int((hist * lens).sum())
                blk.eob_bit = bits.pos
                n = blk.ll_lens[256]
                if bits.take(n) != dc.canonical(blk.ll_lens)[256]:
                    raise DeflateError("the end-of-block code is not where the given text ends")
                blk.text, blk.decoded = bytes(given), False
                if len(out) < 32768:          # a later match may reach back into this text
                    out += blk.text
                else:
                    out = bytearray(out[-32768:]) + blk.text
            else:
                if kind == 2:
                    ll, d = _decoder(blk.ll_lens, "literal/length code"), _decoder(blk.d_lens, "distance code")
                _body(bits, blk, ll, d, out)
        blk.end_bit = bits.pos
        blocks.append(blk)
        if final:
            blk.tail_bits = -bits.pos & 7
            blk.tail_value = bits.take(blk.tail_bits)
            return blocks


def end_byte(blocks):
    """the size in bytes of the stream read_deflate walked"""
    return (blocks[-1].end_bit + blocks[-1].tail_bits) >> 3


def text_of(blocks):
    return b"".join(b.text for b in blocks)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def kdeflate_tokens(ll_lens):
    """the code-length symbol sequence of a K-DEFLATE header for its 257 literal / end-of-block lengths: a non-zero length stands as it is
    (symbol 16 is never used); a run of zeros inside positions 0..255 is cut greedily into pieces of 138 (symbol 18), then one piece of
    11..137 (18) or of 3..10 (17) or one or two single zeros; position 256 is never zero; the one distance length behind it is a zero of
    its own -> [(symbol, extra value)]"""
    assert len(ll_lens) == 257 and ll_lens[256], "257 lengths, the end-of-block code among them"
    out, s = [], 0
    while s < 256:
        if ll_lens[s]:
            out.append((ll_lens[s], 0))
            s += 1
            continue
        e = s
        while e < 256 and not ll_lens[e]:
            e += 1
        run = e - s
        while run >= 138:
            out.append((18, 138 - 11))
            run -= 138
        if run >= 11:
            out.append((18, run - 11))
        elif run >= 3:
            out.append((17, run - 3))
        else:
            out += [(0, 0)] * run
        s = e
    return out + [(ll_lens[256], 0), (0, 0)]


def kdeflate_blocks(text, ll_lens_per_block, block_in, tokens=kdeflate_tokens):
    """the writer's blocks of one raw stream: a dynamic block and an empty stored block per block_in bytes, the empty final fixed block"""
    blocks = []
    pieces = [text[at:at + block_in] for at in range(0, len(text), block_in)]
    assert len(pieces) == len(ll_lens_per_block), (len(pieces), len(ll_lens_per_block))
    for piece, lens in zip(pieces, ll_lens_per_block):
        lens = [int(v) for v in lens]
        blocks += [dc.Dynamic(list(piece), lens, [0], cl_symbols=tokens(lens), cl_lens=KD_CL_LENS, hclen=19), dc.Stored(b"")]
    return blocks + [dc.Fixed([], final=True)]


def bgzf_member(raw, text):
    bsize = 18 + len(raw) + 8
    assert bsize <= 65536, bsize
    return bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + (bsize - 1).to_bytes(2, "little") + raw + \
        zlib.crc32(text).to_bytes(4, "little") + len(text).to_bytes(4, "little")


def kdeflate_model(text, ll_lens_per_block, block_in=65536, container="gzip", tokens=kdeflate_tokens):
    """the bytes K-DEFLATE writes for `text` when block k gets the code lengths ll_lens_per_block[k] (257 each).  container: "gzip" (one
    member), "raw" (its bare stream) or "bgzf" (one member per block, each a stream of its own, and the 28-byte end-of-file block)"""
    text = bytes(text)
    if container == "bgzf":
        out = []
        for k, at in enumerate(range(0, len(text), block_in)):
            piece = text[at:at + block_in]
            raw, t = dc.deflate(kdeflate_blocks(piece, [ll_lens_per_block[k]], block_in, tokens))
            assert t == piece
            out.append(bgzf_member(raw, piece))
        return b"".join(out) + BGZF_EOF
    raw, t = dc.deflate(kdeflate_blocks(text, ll_lens_per_block, block_in, tokens))
    assert t == text
    return raw if container == "raw" else dc.gzip_member(raw, text)


def payloads(data, container):
    """the raw streams inside a container, in order -> [(raw, CRC-32 or None, ISIZE or None)]; the BGZF end-of-file block is checked and left out"""
    if container == "raw":
        return [(data, None, None)]
    if container == "gzip":
        assert data[:10] == bytes([31, 139, 8, 0, 0, 0, 0, 0, 0, 255]), data[:10]
        return [(data[10:-8], int.from_bytes(data[-8:-4], "little"), int.from_bytes(data[-4:], "little"))]
    members = dc.bgzf_blocks(data)
    assert members and members[-1] == BGZF_EOF, "no end-of-file block"
    return [(m[18:-8], int.from_bytes(m[-8:-4], "little"), int.from_bytes(m[-4:], "little")) for m in members[:-1]]


# ---- what code lengths are held against -----------------------------------------------------------------------------------------------
def optimal_cost(hist):
    """bits of the text under a minimum-redundancy (Huffman) code of its histogram, no limit on the depth: the sum of the inner nodes' weights"""
    heap = [int(f) for f in hist if f]
    assert len(heap) >= 2
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a = heapq.heappop(heap) + heapq.heappop(heap)
        cost += a
        heapq.heappush(heap, a)
    return cost


def cost_of(hist, lens):
    return int(sum(int(f) * int(n) for f, n in zip(hist, lens)))


def kraft(lens, limit=15):
    """sum of 2^(limit - len) over the codes: 2^limit for a complete code"""
    return sum(1 << (limit - int(n)) for n in lens if n)


def package_merge(hist, limit):
    """optimal code lengths under a depth limit (Larmore & Hirschberg's package-merge, the plain O(n * limit) list form): `limit` rounds of
    "pair up the list, merge the pairs with the leaves"; the cheapest 2 n - 2 items of the last list count, a symbol's length is the number
    of them it is in"""
    used = sorted((int(f), s) for s, f in enumerate(hist) if f)
    n = len(used)
    assert n >= 2 and (1 << limit) >= n
    leaves = [(f, np.eye(1, n, k, dtype=np.int64)[0]) for k, (f, _) in enumerate(used)]
    cur = list(leaves)
    for _ in range(limit - 1):
        packs = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + packs, key=lambda it: it[0])
    depth = sum(it[1] for it in cur[:2 * n - 2])
    lens = [0] * len(hist)
    for k, (_, s) in enumerate(used):
        lens[s] = int(depth[k])
    return lens


def kdeflate_lengths(hist, limit=15):
    """a plain rendering of the rule K-DEFLATE's comment states, for the tests that run without the device: the used symbols sorted by
    (frequency, symbol), the in-place minimum-redundancy algorithm of Moffat & Katajainen over them, and while the longest code exceeds
    `limit` every frequency halved (rounded up) and the tree built again -> (lengths by symbol, number of halvings).  The device's own
    lengths are never replaced by these."""
    used = sorted((int(f), s) for s, f in enumerate(hist) if f)
    n = len(used)
    assert n >= 2
    freq, halvings = [f for f, _ in used], 0
    while True:
        a = list(freq)
        a[0] += a[1]
        root, leaf = 0, 2
        for nxt in range(1, n - 1):
            if leaf >= n or a[root] < a[leaf]:
                a[nxt] = a[root]
                a[root] = nxt
                root += 1
            else:
                a[nxt] = a[leaf]
                leaf += 1
            if leaf >= n or (root < nxt and a[root] < a[leaf]):
                a[nxt] += a[root]
                a[root] = nxt
                root += 1
            else:
                a[nxt] += a[leaf]
                leaf += 1
        a[n - 2] = 0
        for nxt in range(n - 3, -1, -1):
            a[nxt] = a[a[nxt]] + 1
        avbl, taken, dpth, root, nxt = 1, 0, 0, n - 2, n - 1
        while avbl > 0:
            while root >= 0 and a[root] == dpth:
                taken += 1
                root -= 1
            while avbl > taken:
                a[nxt] = dpth
                nxt -= 1
                avbl -= 1
            avbl, dpth, taken = 2 * taken, dpth + 1, 0
        if a[0] <= limit:
            lens = [0] * len(hist)
            for k, (_, s) in enumerate(used):
                lens[s] = a[k]
            return lens, halvings
        freq = [(f + 1) >> 1 for f in freq]
        halvings += 1
