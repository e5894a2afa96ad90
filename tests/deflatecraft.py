"""A DEFLATE writer for tests (RFC 1951 / RFC 1952), pure Python and independent of the project: a list of blocks -> the raw stream and the
text it must inflate to.  Every stream the project's other tests read was written by zlib's compressor, which never emits a distance above
32506, a single distance code, a code-length repeat across the two alphabets and much else that is legal; the streams here are written bit
by bit instead.  The expected text comes from `expand` (the token expander below), never from a decoder; the tests hold zlib's inflater
against it first (legality and content) and the project's two decoders second.

A token is a literal byte (int), a match `(length, distance)`, `("sym", s)` (the bare literal/length symbol s: for symbols that may not
occur) or `("raw", value, n_bits)` (bits as they are, least significant first: for distance codes that do not exist).

`catalogue()` returns the named cases both test files use."""
import heapq
import random
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def len_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3 .. 258"""
    if length == 258:
        return 285, 0, 0
    i = max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_symbol(dist):
    """(symbol, extra bits, extra value) of a match distance 1 .. 32768"""
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


_LEN_SYM = {n: len_symbol(n) for n in range(3, 259)}


def rev(value, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (value & 1)
        value >>= 1
    return r


def canonical(lens):
    """canonical Huffman codes (RFC 1951 3.2.2) of the code lengths, bit-reversed, i.e. as they go into the stream least significant bit first"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for n in lens:
        if not n:
            out.append(0)
            continue
        out.append(rev(nxt[n] & ((1 << n) - 1), n))
        nxt[n] += 1
    return out


def huff_lengths(freqs, limit):
    """code lengths of a complete Huffman code over the symbols with freqs > 0, none longer than `limit` (the frequencies are halved until
    the code fits); a single used symbol gets a second one beside it, as zlib's compressor does, so that the code is complete"""
    freqs = list(freqs)
    used = [s for s, f in enumerate(freqs) if f]
    if len(used) < 2:
        for s in range(len(freqs)):
            if len(used) < 2 and s not in used:
                used.append(s)
                freqs[s] = 1
    shift = 0
    while True:
        heap = [(max(1, freqs[s] >> shift), s, (s,)) for s in used]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        while len(heap) > 1:
            fa, ka, a = heapq.heappop(heap)
            fb, kb, b = heapq.heappop(heap)
            for s in a + b:
                depth[s] += 1
            heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
        if max(depth.values()) <= limit:
            lens = [0] * len(freqs)
            for s, d in depth.items():
                lens[s] = d
            return lens
        shift += 1


class BitWriter:
    """bits gathered in an int, whole bytes moved to a bytearray as they fill up"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, n_bits):
        self.acc |= (value & ((1 << n_bits) - 1)) << self.n
        self.n += n_bits
        if self.n >= 64:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def align(self):
        if self.n & 7:
            self.put(0, 8 - (self.n & 7))

    def put_bytes(self, data):
        self.align()
        self.flush()
        self.out += data

    def flush(self):
        k = (self.n + 7) >> 3
        self.out += self.acc.to_bytes(k, "little")
        self.acc = 0
        self.n = 0

    @property
    def bit_pos(self):
        return 8 * len(self.out) + self.n

    def getvalue(self):
        self.flush()
        return bytes(self.out)


def expand(tokens, out):
    """the text of a token list behind the text so far (`out`, a bytearray, grows): the 10-line reference of what a stream means"""
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif not isinstance(t[0], str):
            length, dist = t
            assert 3 <= length <= 258 and 1 <= dist <= min(32768, len(out)), (t, len(out))
            for _ in range(length):
                out.append(out[-dist])
    return out


def _put_tokens(bw, tokens, ll_lens, d_lens, marks=None):
    ll, d = canonical(ll_lens), canonical(d_lens)
    for t in tokens:
        if marks is not None:
            marks.append(bw.bit_pos)
        if isinstance(t, int):
            assert ll_lens[t], ("no code for literal", t)
            bw.put(ll[t], ll_lens[t])
        elif t[0] == "sym":
            bw.put(ll[t[1]], ll_lens[t[1]])
        elif t[0] == "raw":
            bw.put(t[1], t[2])
        else:
            s, xb, xv = _LEN_SYM[t[0]]
            assert ll_lens[s], ("no code for length symbol", s)
            bw.put(ll[s], ll_lens[s])
            bw.put(xv, xb)
            s, xb, xv = dist_symbol(t[1])
            assert d_lens[s], ("no code for distance symbol", s)
            bw.put(d[s], d_lens[s])
            bw.put(xv, xb)
    eob_at = bw.bit_pos
    bw.put(ll[256], ll_lens[256])
    return eob_at


class Stored:
    def __init__(self, data, final=False, nlen=None):
        assert len(data) <= 65535
        self.data, self.final, self.nlen = bytes(data), final, nlen

    def emit(self, bw, text):
        bw.put(1 if self.final else 0, 1)
        bw.put(0, 2)
        n = len(self.data)
        bw.put_bytes(n.to_bytes(2, "little") + ((n ^ 0xFFFF) if self.nlen is None else self.nlen).to_bytes(2, "little") + self.data)
        text += self.data


class Fixed:
    def __init__(self, tokens, final=False, meaningless=False):
        self.tokens, self.final, self.marks, self.meaningless = list(tokens), final, [], meaningless

    def emit(self, bw, text):
        bw.put(1 if self.final else 0, 1)
        bw.put(1, 2)
        self.eob_at = _put_tokens(bw, self.tokens, FIXED_LL, FIXED_D, self.marks)
        if not self.meaningless:         # (the tokens of an illegal stream are written, not expanded)
            expand(self.tokens, text)


def plain_symbols(lens):
    """code-length symbol sequence without repeats: [(symbol, extra value)]"""
    return [(n, 0) for n in lens]


def run_symbols(lens):
    """code-length symbol sequence with 16 / 17 / 18 runs over the whole array (literal/length and distance lengths as one array, so a run
    crosses the boundary where the values allow it)"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
        i = j
    return out


_CL_EXTRA = {16: 2, 17: 3, 18: 7}


class Dynamic:
    """ll_lens / d_lens: the code lengths the header says (hlit and hdist entries unless hlit_field / hdist_field say another count).
    cl_symbols: the header's code-length symbol sequence [(symbol, extra value)], default run_symbols over both arrays; cl_lens: the lengths
    of the code-length code by symbol (default: Huffman over the sequence, at most 7 bits); hclen: how many of them are written;
    hlit_field / hdist_field: the header's two count fields as written, where they should not match the arrays."""

    def __init__(self, tokens, ll_lens, d_lens, final=False, cl_symbols=None, cl_lens=None, hclen=None, hlit_field=None, hdist_field=None,
                 meaningless=False):
        self.tokens, self.final, self.marks, self.meaningless = list(tokens), final, [], meaningless
        self.ll_lens, self.d_lens = list(ll_lens), list(d_lens)
        assert 257 <= len(self.ll_lens) <= 288 and 1 <= len(self.d_lens) <= 32
        self.cl_symbols = run_symbols(self.ll_lens + self.d_lens) if cl_symbols is None else list(cl_symbols)
        if cl_lens is None:
            f = [0] * 19
            for s, _ in self.cl_symbols:
                f[s] += 1
            cl_lens = huff_lengths(f, 7)
        self.cl_lens = list(cl_lens)
        self.hclen = max(4, max(k + 1 for k in range(19) if self.cl_lens[CL_ORDER[k]])) if hclen is None else hclen
        self.hlit_field = len(self.ll_lens) - 257 if hlit_field is None else hlit_field
        self.hdist_field = len(self.d_lens) - 1 if hdist_field is None else hdist_field

    def emit(self, bw, text):
        bw.put(1 if self.final else 0, 1)
        bw.put(2, 2)
        bw.put(self.hlit_field, 5)
        bw.put(self.hdist_field, 5)
        bw.put(self.hclen - 4, 4)
        for k in range(self.hclen):
            bw.put(self.cl_lens[CL_ORDER[k]], 3)
        cl = canonical(self.cl_lens)
        for s, x in self.cl_symbols:
            bw.put(cl[s], self.cl_lens[s])
            if s >= 16:
                bw.put(x, _CL_EXTRA[s])
        self.eob_at = _put_tokens(bw, self.tokens, self.ll_lens + [0] * (288 - len(self.ll_lens)), self.d_lens + [0] * (32 - len(self.d_lens)), self.marks)
        if not self.meaningless:
            expand(self.tokens, text)


class Reserved:
    """block type 3"""
    final = True

    def emit(self, bw, text):
        bw.put(1, 1)
        bw.put(3, 2)
        bw.put(0, 13)


def deflate(blocks):
    """-> (raw DEFLATE stream, the text it stands for)"""
    bw, text = BitWriter(), bytearray()
    for b in blocks:
        b.emit(bw, text)
    return bw.getvalue(), bytes(text)


def steps_of(block):
    """the tokens of a written block as a decoder sees them that takes, step by step, the tokens starting within 64 bits of the step's first
    one (K-INFLATE: lane = bit offset in the step; a block's first token starts a step, and so does the first token 64 bits or more
    behind a step's start) -> list of steps, each the list of its tokens' bit positions in the raw stream, the end-of-block code included"""
    steps = []
    for m in block.marks + [block.eob_at]:
        if not steps or m - steps[-1][0] >= 64:
            steps.append([])
        steps[-1].append(m)
    return steps


def gzip_member(raw, text, ftext=False, fhcrc=False, extra=None, name=None, comment=None, crc=None, isize=None):
    """one RFC 1952 member around a raw stream; CRC-32 and ISIZE of `text` unless given"""
    flg = (1 if ftext else 0) | (2 if fhcrc else 0) | (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0)
    head = bytes([31, 139, 8, flg, 0, 0, 0, 0, 0, 255])
    if extra is not None:
        head += len(extra).to_bytes(2, "little") + extra
    if name is not None:
        assert 0 not in name
        head += name + b"\0"
    if comment is not None:
        assert 0 not in comment
        head += comment + b"\0"
    if fhcrc:
        head += (zlib.crc32(head) & 0xFFFF).to_bytes(2, "little")
    c = zlib.crc32(text) if crc is None else crc
    n = len(text) if isize is None else isize
    return head + raw + c.to_bytes(4, "little") + (n & 0xFFFFFFFF).to_bytes(4, "little")


def gunzip_reference(data):
    """zlib's inflater over every member of a gzip file (zlib.decompressobj(31) per member) -> (text, members); zlib.error for a member that
    is malformed or does not end.  Zero bytes behind the last member are padding."""
    out, n = [], 0
    while data:
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        if not d.eof:
            raise zlib.error("incomplete or truncated stream")
        n += 1
        data = d.unused_data
        if not data.strip(b"\0"):
            break
    return b"".join(out), n


class Case:
    """one file of the catalogue.  text: what it must inflate to (None: it must be refused); raw: its bare DEFLATE stream when it is one
    member (for zlib.decompress(raw, -15)); n_members where the case fixes it; device_refuses: legal, but more than K-INFLATE takes (the
    host decoder reads it); room: for an illegal file, an output capacity that is more than the text in front of what makes it illegal, so
    that a decoder given that much is not stopped by the capacity first; big: the file is of about 1 MB or more; blocks: the writer's
    blocks `raw` was made of, where the case kept them (a reader's view of the stream is held against them)"""

    def __init__(self, name, file, text, raw=None, n_members=None, device_refuses=False, big=False, room=4096, blocks=None):
        self.name, self.file, self.text, self.raw, self.n_members, self.device_refuses, self.big = name, file, text, raw, n_members, device_refuses, big
        self.room, self.blocks = room, blocks

    def __repr__(self):
        return f"Case({self.name})"


def _single(name, blocks, **header):
    raw, text = deflate(blocks)
    return Case(name, gzip_member(raw, text, **header), text, raw=raw, n_members=1, blocks=list(blocks))


def _literals(rng, n, alphabet=None):
    return list(rng.randbytes(n)) if alphabet is None else [alphabet[b & 3] for b in rng.randbytes(n)]


def lens_of(n, assign):
    lens = [0] * n
    for s, v in assign.items():
        lens[s] = v
    return lens


FAR_MATCHES = [(258, 32768), (3, 32768), (258, 32767), (258, 32507), (258, 1), (4, 2), (258, 7), (9, 8), (258, 9)]


def dynamic_for(tokens, final=True, **kw):
    """a dynamic block whose two codes are Huffman codes of the tokens' own frequencies, at most 15 bits"""
    fl, fd = [0] * 286, [0] * 30
    fl[256] = 1
    for t in tokens:
        if isinstance(t, int):
            fl[t] += 1
        else:
            fl[_LEN_SYM[t[0]][0]] += 1
            fd[dist_symbol(t[1])[0]] += 1
    ll = huff_lengths(fl, 15)
    d = huff_lengths(fd, 15)
    while len(ll) > 257 and not ll[-1]:
        ll.pop()
    while len(d) > 1 and not d[-1]:
        d.pop()
    return Dynamic(tokens, ll, d, final=final, **kw)


def far_cases():
    rng = random.Random(32768)
    lits = _literals(rng, 32768)
    toks = lits + FAR_MATCHES
    out = [_single("far/fixed", [Fixed(toks, final=True)]), _single("far/dynamic", [dynamic_for(toks)])]
    # the literals from a stored block, and every match in a block of its own: it is the only token with output in its 64-bit step, the
    # step starts on a multiple of the ring size, and the ring slot a byte is read from is the slot it is written to
    out.append(_single("far/stored+fixed", [Stored(bytes(lits)), Fixed(FAR_MATCHES, final=True)]))
    blocks = [Stored(bytes(lits))]
    for k, m in enumerate(FAR_MATCHES):
        blocks.append(Fixed([m]) if k % 2 else dynamic_for([m], final=False))
    blocks.append(Fixed([], final=True))
    out.append(_single("far/stored+one_match_per_block", blocks))
    return out


def one_dist_code_cases():
    # literal A with 1 bit, end of block and length 258 with 2 bits each; ONE distance code of one bit (an incomplete code inflate accepts)
    ll = lens_of(286, {65: 1, 256: 2, 285: 2})
    a = _single("one_dist_code/single_1bit", [Dynamic([65, (258, 1), (258, 1)], ll, [1], final=True)])
    # HDIST = 1 and that one length 0: no distance code at all, literals only
    rng = random.Random(7)
    lits = _literals(rng, 3000, b"ACGT")
    ll2 = lens_of(257, {65: 2, 67: 2, 71: 2, 84: 3, 256: 3})
    b = _single("one_dist_code/no_dist_code", [Dynamic(lits, ll2, [0], final=True)])
    return [a, b]


def eob_only_cases():
    empty = Dynamic([], lens_of(257, {256: 1}), [0])        # its only code is a 1-bit end of block
    a = _single("eob_only/stored_then_match", [empty, Stored(b""), Stored(b"GATTACA"), Fixed([(7, 7), (258, 14)], final=True)])
    rng = random.Random(65535)
    b = _single("eob_only/stored_65535_then_match", [Stored(rng.randbytes(65535)), Fixed([(258, 30000)], final=True)])
    return [a, b]


def repeat_across_cases():
    out = []
    rng = random.Random(257)
    lits = _literals(rng, 4000)
    # HLIT = 257.  255 literals of 8 bits, literal 255 and the end of block of 9; distances 9, 9 and 1 .. 8: a symbol-16 repeat of the 9
    # covers indices 256, 257, 258 (the last literal/length length and the first two distance lengths)
    ll, d = [8] * 255 + [9, 9], [9, 9, 1, 2, 3, 4, 5, 6, 7, 8]
    syms = [(8, 0)] + [(16, 3)] * 42 + [(8, 0), (8, 0)] + [(9, 0), (16, 0)] + plain_symbols(d[2:])      # 1 + 42 * 6 + 2 = 255 eights
    out.append(_single("repeat_across/16_from_256", [Dynamic(lits, ll, d, final=True, cl_symbols=syms)]))
    # the repeat STARTS at index 257: its value is the last literal/length length
    d = [9, 9, 9, 9, 1, 2, 3, 4, 5, 6, 7]
    syms = [(8, 0)] + [(16, 3)] * 42 + [(8, 0), (8, 0)] + [(9, 0), (9, 0), (16, 1)] + plain_symbols(d[4:])
    out.append(_single("repeat_across/16_from_257", [Dynamic(lits, ll, d, final=True, cl_symbols=syms)]))
    # a symbol-18 zero run from the unused length symbols into the distance lengths (HLIT = 270: index 256 must have a code)
    ll = [8] * 254 + [9, 9, 9, 9] + [0] * 12
    d = [0] * 10 + [1, 1]
    syms = [(8, 0)] + [(16, 3)] * 42 + [(8, 0)] + [(9, 0), (16, 0)] + [(18, 22 - 11)] + [(1, 0), (1, 0)]    # 254 eights, four nines, 22 zeros
    toks = lits[:300]
    for k in range(200):
        toks += [(3, 33 + rng.randrange(32)), lits[k]]
    out.append(_single("repeat_across/18_zero_run", [Dynamic(toks, ll, d, final=True, cl_symbols=syms)]))
    return out


def deep_codes_block(final=True, n_wide=420, seed=48):
    """HLIT = 286, HDIST = 30, HCLEN = 19; both codes are the chain 1, 2, ..., 14, 15, 15.  The widest token: the 15-bit length symbol 284
    (5 extra bits) and the 15-bit distance symbol 29 (13 extra bits) = 48 bits"""
    chain_ll = [65, 256, 67, 71, 84, 78, 10, 43, 64, 48, 49, 50, 257, 265, 122, 284]      # lengths 1 .. 14, 15, 15 (z and 284 have 15 bits)
    ll = lens_of(286, {s: min(k + 1, 15) for k, s in enumerate(chain_ll)})
    d = [0] * 14 + list(range(1, 14)) + [15, 14, 15]                                      # codes 14 .. 26: 1 .. 13; 27: 15, 28: 14, 29: 15
    rng = random.Random(seed)
    toks = [65] * 24600 + [67, 71, 84, 78, 122] * 8
    for k in range(n_wide):
        toks += [65] * rng.randrange(0, 12)
        toks.append((227 + rng.randrange(31), 24577 + rng.randrange(35)))                # 15 + 5 + 15 + 13 bits
        if k % 3 == 0:
            toks.append(122)                                                             # the 15-bit literal
        if k % 5 == 0:
            toks.append((11 + rng.randrange(2), 16385 + rng.randrange(8192)))           # 14 + 1 + 14 + 13 bits
        if k % 7 == 0:
            toks.append((3, 12289 + rng.randrange(4096)))                                # 13 + 15 + 12 bits
    return Dynamic(toks, ll, d, final=final, hclen=19)


def deep_codes_cases():
    blk = deep_codes_block()
    case = _single("deep_codes", [blk])
    wide = [m for t, m in zip(blk.tokens, blk.marks) if not isinstance(t, int) and t[0] >= 227]
    assert len({m % 64 for m in wide}) == 64, "the 48-bit tokens must start at every bit offset modulo 64"
    # K-INFLATE stages 4096 bits of input and stages again, from the step's 32-bit word on, before a step whose lanes' 160 bits would leave them
    # (the stream starts behind the 10-byte member header).  A token is never split by that; what can go wrong is the first step read from
    # the new words and the last one read from the old: 48-bit tokens in both, several times
    wide, base, after, before, last = set(wide), None, 0, 0, []
    for step in steps_of(blk):
        at = step[0] + 80
        if base is None or at - base + 160 > 4096:
            if base is not None and wide.intersection(step):
                after += 1
            if base is not None and wide.intersection(last):
                before += 1
            base = at & ~31
        last = step
    assert after >= 3 and before >= 3, ("48-bit tokens around the re-staging of the input", after, before)
    return [case]


def dense_steps_block(final=True, n=40):
    # length 258 with ONE bit and distance 1 with one bit: a (258, 1) match is 2 bits, a 64-bit step makes 32 * 258 bytes
    ll = lens_of(286, {285: 1, 65: 2, 256: 3, 67: 4, 71: 5, 84: 5})
    d = lens_of(13, {0: 1, 1: 2, 11: 3, 12: 3})
    rng = random.Random(258)
    toks = _literals(rng, 70, b"ACGT") + [(258, 1)] * 70
    for dist in (2, 63, 64, 65, 1, 64, 2, 65, 63):
        toks += _literals(rng, 67, b"ACGT") + [(258, dist)] * n
    return Dynamic(toks, ll, d, final=final)


def block_seams_cases():
    rng = random.Random(300)
    blocks = []
    small = lens_of(257, {65: 1, 67: 2, 256: 3, 71: 3})
    for k in range(300):
        kind = k % 4
        if kind == 0:
            blocks.append(Fixed([]))
        elif kind == 1:
            blocks.append(Fixed([rng.randrange(256)]))
        elif kind == 2:
            blocks.append(Stored(rng.randbytes((k // 4) % 3)))
        else:
            # 0 .. 70 one-bit literals (and a few of two and three bits in front of some): the end of block on every lane of the first step
            # and on the first lanes of a second one
            blocks.append(Dynamic(_literals(rng, (k // 4) % 5, b"ACGA") * (k >= 288) + [65] * ((k // 4) % 72), small, [0]))
    blocks[-1].final = True
    case = _single("block_seams", blocks)
    ends = {(len(st) - 1, b.eob_at - st[-1][0]) for b in blocks if not isinstance(b, Stored) for st in [steps_of(b)]}
    assert {(0, lane) for lane in range(64)} | {(1, 0), (1, 1)} <= ends, "the end-of-block code must land on every lane"
    return [case]


def soup_tokens(seed, n_text=100_000):
    rng = random.Random(seed)
    dists = list(range(1, 10)) + [15, 16, 17, 63, 64, 65, 257, 4097, 24577, 32767, 32768, None]
    lengths = [3, 4, 8, 9, 10, 11, 64, 65, 257, 258, None]
    toks, n = [], 0
    skew = bytes(min(255, int(rng.expovariate(0.03))) for _ in range(4096))
    while n < n_text:
        if n < 300 or rng.random() < 0.45:
            k = rng.randrange(1, 40)
            toks += [skew[rng.randrange(4096)] for _ in range(k)]
            n += k
        else:
            dist = rng.choice(dists) or rng.randrange(1, 32769)
            length = rng.choice(lengths) or rng.randrange(3, 259)
            toks.append((length, min(dist, n)))
            n += length
    return toks


def soup_cases():
    out = []
    for k in range(6):
        toks = soup_tokens(1000 + k)
        out.append(_single(f"soup/{k}_{'fixed' if k % 2 else 'dynamic'}", [Fixed(toks, final=True) if k % 2 else dynamic_for(toks)]))
    return out


def headers_cases():
    toks = soup_tokens(77, 2000)
    blocks = [dynamic_for(toks)]
    raw, text = deflate(blocks)
    pattern = b"\x1f\x8b\x08\x01\x02"
    extras = [b"", b"extra", (pattern * 13107)[:65535]]
    out, k = [], 0
    for bits in range(32):
        kw = dict(ftext=bool(bits & 1), fhcrc=bool(bits & 2))
        if bits & 4:
            kw["extra"] = extras[k % 3]
            k += 1
        if bits & 8:
            kw["name"] = b"reads\x1f\x8b\x08_0001.fastq"
        if bits & 16:
            kw["comment"] = b"a comment \x1f\x8b and more"
        out.append(Case(f"headers/flg{bits:02x}" + (f"_x{len(kw['extra'])}" if bits & 4 else ""), gzip_member(raw, text, **kw), text, raw=raw, n_members=1,
                        blocks=blocks))
    return out


def fastq_text(n_bytes, seed):
    rng = random.Random(seed)
    acgt = bytes(b"ACGT"[b & 3] for b in range(256))
    qual = bytes(35 + (b % 40) for b in range(256))
    recs, n, i = [], 0, 0
    while n < n_bytes:
        m = rng.randrange(200, 1500)
        r = b"@%08x-aaaa-bbbb-cccc-%012x runid=abcdef read=%d ch=%d\n" % (i * 2654435761 % 2 ** 32, i, i, i % 512) + \
            rng.randbytes(m).translate(acgt) + b"\n+\n" + rng.randbytes(m).translate(qual) + b"\n"
        recs.append(r)
        n += len(r)
        i += 1
    return b"".join(recs)


def bgzf_blocks(data):
    """the members of a BGZF file by their BSIZE fields -> list of bytes"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00"
        n = int.from_bytes(data[at + 16:at + 18], "little") + 1
        out.append(data[at:at + n])
        at += n
    return out


def bgzf_fastq_cases(bgzf_deflate, block_bytes=11_000):
    """bgzf_deflate(text, block_bytes) -> the BGZF file (the project's own writer, handed in by the caller: this module imports nothing of it)"""
    text = fastq_text(3_000_000, 64)
    blocks = bgzf_blocks(bytes(bgzf_deflate(text, block_bytes)))
    assert len(blocks) > 258 and len(blocks[-1]) == 28
    a = Case("bgzf_fastq/256_members", b"".join(blocks[:255]) + blocks[-1], text[:255 * block_bytes], n_members=256, big=True)
    b = Case("bgzf_fastq/257_members", b"".join(blocks[:256]) + blocks[-1], text[:256 * block_bytes], n_members=257, device_refuses=True, big=True)
    return [a, b]


def stored_member(text, **kw):
    blocks = [Stored(text[at:at + 65535]) for at in range(0, len(text), 65535)] or [Stored(b"")]
    blocks[-1].final = True
    raw, t = deflate(blocks)
    assert t == text
    return gzip_member(raw, text, **kw)


def crc_pieces_cases():
    rng = random.Random(1 << 20)
    out = []
    for n in (1_048_575, 1_048_576, 1_048_577, 2_097_153, 1, 255, 256, 257):
        text = rng.randbytes(n)
        out.append(Case(f"crc_pieces/{n}", stored_member(text), text, n_members=1, big=n > 1_000_000))
    parts = [rng.randbytes(70_000), rng.randbytes(1), rng.randbytes(1_048_577)]
    out.append(Case("crc_pieces/three_members", b"".join(stored_member(p) for p in parts), b"".join(parts), n_members=3, big=True))
    return out


def legal_cases(bgzf_deflate=None):
    cases = far_cases() + one_dist_code_cases() + eob_only_cases() + repeat_across_cases() + deep_codes_cases()
    cases.append(_single("dense_steps", [dense_steps_block()]))
    cases += block_seams_cases() + soup_cases() + headers_cases() + crc_pieces_cases()
    if bgzf_deflate is not None:
        cases += bgzf_fastq_cases(bgzf_deflate)
    return cases


def _bad(name, blocks, cut=None):
    raw, _ = deflate(blocks)
    if cut is not None:
        raw = raw[:cut]
        return Case("illegal/" + name, gzip_member(raw, b"")[:-8], None, raw=raw)      # the file ends where the stream was cut
    return Case("illegal/" + name, gzip_member(raw, b""), None, raw=raw)


def illegal_cases():
    """streams both decoders must refuse; zlib's inflater refuses every one of them (the self-test asserts it).  The trailer of
    distance_into_previous_member and of the CRC case is the one a decoder that went on would confirm.  The other trailers are those of the
    empty text: where the tokens in front of the illegal one make text (symbols 286 / 287, distance codes 30 / 31, no end-of-block code, no
    distance code), a decoder that took the illegal token would still be refused by the trailer, so the tests ask these files for the
    KIND of refusal (a bad code, not a bad CRC) and not only for one"""
    out = []
    lits = list(b"ACGTACGTAC")
    out.append(_bad("distance_1_beyond_start", [Fixed(lits + [("sym", 257), ("raw", rev(dist_symbol(11)[0], 5), 5), ("raw", 2, 2)], final=True, meaningless=True)]))   # (3, 11) behind 10 bytes
    # the second member's match reaches into the first member's text: every member starts with an empty window
    good_raw, good_text = deflate([Fixed(list(b"x" * 100), final=True)])
    bad_raw, _ = deflate([Fixed([65, ("sym", 257), ("raw", rev(dist_symbol(50)[0], 5), 5), ("raw", 50 - 49, 4)], final=True, meaningless=True)])
    # (the trailer is the one a decoder that does reach back would confirm: only the distance check stands between this file and status 0)
    out.append(Case("illegal/distance_into_previous_member", gzip_member(good_raw, good_text) + gzip_member(bad_raw, b"Axxx"), None))
    for s in (286, 287):
        out.append(_bad(f"fixed_symbol_{s}", [Fixed(lits + [("sym", s), ("raw", 0, 5)] + lits, final=True, meaningless=True)]))
    for s in (30, 31):
        out.append(_bad(f"fixed_distance_code_{s}", [Fixed(lits + [("sym", 257), ("raw", rev(s, 5), 5)] + lits, final=True, meaningless=True)]))
    out.append(_bad("oversubscribed_literal_code", [Dynamic([], lens_of(257, {65: 1, 66: 1, 256: 1}), [1, 1], final=True)]))
    out.append(_bad("incomplete_literal_code_two_codes", [Dynamic([], lens_of(257, {65: 2, 256: 2}), [1, 1], final=True)]))
    ll = lens_of(257, {65: 1, 256: 1})
    out.append(_bad("incomplete_code_length_code", [Dynamic([], ll, [1, 1], final=True, cl_symbols=plain_symbols(ll + [1, 1]),
                                                                      cl_lens=lens_of(19, {0: 2, 1: 2}))]))
    out.append(_bad("missing_end_of_block_code", [Dynamic([65, 66], lens_of(257, {65: 1, 66: 1}), [1, 1], final=True)]))
    out.append(_bad("hlit_287", [Dynamic([], ll, [1, 1], final=True, hlit_field=30)]))
    out.append(_bad("hdist_31", [Dynamic([], ll, [1, 1], final=True, hdist_field=30)]))
    seq = run_symbols(ll + [1, 1])
    cl = lens_of(19, {0: 2, 1: 2, 16: 3, 17: 3, 18: 2})
    out.append(_bad("repeat_16_first", [Dynamic([], ll, [1, 1], final=True, cl_symbols=[(16, 0)] + seq, cl_lens=cl)]))
    out.append(_bad("repeat_past_the_end", [Dynamic([], ll, [1, 1], final=True, cl_symbols=plain_symbols(ll) + [(1, 0), (18, 0)], cl_lens=cl)]))
    # a match in a block whose distance alphabet has no code (any bit behind the length symbol is "a distance code")
    ll3 = lens_of(258, {65: 1, 256: 2, 257: 2})
    out.append(_bad("match_without_distance_code", [Dynamic([65, 65, 65, ("sym", 257), ("raw", 0, 1), 65], ll3, [0], final=True, meaningless=True)]))
    out.append(_bad("stored_len_nlen_mismatch", [Stored(b"hello", final=True, nlen=0)]))
    out.append(_bad("reserved_block_type", [Reserved()]))
    deep = deep_codes_block()
    deflate([deep])
    wide = [m for t, m in zip(deep.tokens, deep.marks) if not isinstance(t, int) and t[0] >= 227]
    m = next(m for m in wide[60:] if (m + 20) % 8 == 0)
    made = len(expand(deep.tokens[:deep.marks.index(m)], bytearray()))                     # the text in front of the token that is cut
    out.append(_bad("cut_inside_a_48_bit_token", [deep_codes_block()], cut=(m + 20) // 8))
    out[-1].room = made + 1024
    assert zlib.decompressobj(-15).decompress(out[-1].raw) == expand(deep.tokens[:deep.marks.index(m)], bytearray()) and made > 32768
    out.append(_bad("cut_inside_a_dynamic_header", [deep_codes_block()], cut=20))
    # a member of 1 MiB + 1 byte with one text bit changed in its last byte and the trailer left alone: the last CRC piece is one byte
    text = random.Random(8).randbytes(1_048_577)
    flipped = text[:-1] + bytes([text[-1] ^ 0x10])
    out.append(Case("illegal/crc_last_byte_of_1048577", stored_member(flipped, crc=zlib.crc32(text)), None, big=True, room=1_048_577))
    return out


def catalogue(bgzf_deflate=None):
    """-> (legal cases, illegal cases)"""
    return legal_cases(bgzf_deflate), illegal_cases()


_CACHE = {}


def shared_catalogue(bgzf_deflate=None):
    """the catalogue built once per process and shared by the tests that read it (nobody changes it)"""
    key = bgzf_deflate is not None
    if key not in _CACHE:
        _CACHE[key] = catalogue(bgzf_deflate)
    return _CACHE[key]
