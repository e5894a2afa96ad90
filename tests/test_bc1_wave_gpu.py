"""K-BC1's one-kernel table path `k_bc_match_ed1w` (a wave per 64 reads, bucket look-ups in dense rounds) on the GPU: whole records of the default path,
of the two kernels it replaces (`SMI_BC1_TWO_KERNELS=1`) and of the oracle, 3' and 5', on waves built for the numbering (part-full last waves, 0 / 5
/ alternating pairs per read, a hit on either side of a round seam), for invalid windows and windows with an N, for look-ups that walk into a second
bucket, and for the pick's rules."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DS = (-2, -1, 0, 1, 2)            # key-side offsets: the key of d is bases 2 - d .. 17 - d of a 20-base stretch in key orientation
OFFS = (0, -1, 1, -2, 2)          # the reference's order of the record-side offsets o (pair q of a read); d = o for 3', -o for 5'
BASE = {-2: 0, -1: 4, 0: 12, 1: 20, 2: 28}
MASK = {-2: 3, -1: 7, 0: 7, 1: 7, 2: 3}
M32 = np.uint64(0xFFFFFFFF)
U = np.uint64
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 193)


# ---- host models of smi_bc.hip ------------------------------------------------------------------------------------------------------------
def _lowmask(nbits):
    return U(0xFFFFFFFF) if nbits >= 32 else U((1 << nbits) - 1)


def n1_member(k, slot):
    k = np.asarray(k, dtype=np.uint64)
    if slot < 48:
        return k ^ U((slot % 3 + 1) << (30 - 2 * (slot // 3)))
    if slot < 108:
        j = slot - 48
        sh = 30 - 2 * (1 + j // 4)
        return ((k & ~_lowmask(sh + 2)) | ((k & _lowmask(sh)) << U(2)) | U(j & 3)) & M32
    if slot < 168:
        j = slot - 108
        q = j // 4
        top = 32 - 2 * q
        return ((k & ~_lowmask(top) & M32) | U((j & 3) << (30 - 2 * q)) | ((k & _lowmask(top)) >> U(2))) & M32
    return k


def neighbourhood(keys):
    return np.unique(np.concatenate([n1_member(keys, s) for s in range(169)]))


def nbl_cell(key, d):
    sh = 2 * (2 - d)
    core = (key >> U(sh)) & U(0xFFFFFF)
    low = U((1 << sh) - 1)
    flank = ((key >> U(24)) & ~low & U(0xFF)) | (key & low)
    return ((core << U(5)) + U(BASE[d]) + ((flank >> U(5)) & U(MASK[d]))) * U(32) + (flank & U(31))


def nt_bucket(x, cap):
    """nt_slot(x, cap) >> 3: the home bucket of sequence x in a table of cap slots"""
    h = (np.asarray(x, dtype=np.uint64) * U(0x9E3779B1)) & M32
    return (h * U(cap >> 3)) >> U(32)


def key_3p_with_n(window, is_n):
    """make_key's emulation for a 3' window with an N (window orientation, base 0 first): every base before the LAST N reads as T, the N itself as C"""
    w = _pack(window)
    i = int(np.flatnonzero(is_n).max())
    w = (w & _lowmask(30 - 2 * i)) | ((U(0xFFFFFFFF) << U(31 - 2 * i)) & M32)
    return _pack(3 - _bases16(np.array([w]))[0, ::-1])


def _bases16(x):
    return ((np.asarray(x, dtype=np.uint64)[:, None] >> (np.arange(15, -1, -1, dtype=np.uint64) * U(2))) & U(3)).astype(np.uint8)


def _pack(b):
    return (np.asarray(b).astype(np.uint64) << (np.arange(15, -1, -1, dtype=np.uint64) * U(2))).sum(-1)


# ---- reads -------------------------------------------------------------------------------------------------------------------------------
def _records(stretch, five_prime, rng):
    """20-base stretches in key orientation -> (codes [n, 48], ae [n]) as the oracle reads them.  5': the 25-base record starts at codes[6] and its
    bases 0 .. 19 are the stretch (the base a deletion at d appends is stretch[18 - d]; at d = -2 it is codes[26]).  3': the 24-base record starts at
    codes[7] and its bases 4 .. 23 are the stretch's reverse complement (a deletion appends the key's own last base)."""
    n = stretch.shape[0]
    codes = rng.integers(0, 4, (n, 48), dtype=np.uint8)
    if five_prime:
        codes[:, 6:26] = stretch
        ae = np.full(n, 8, dtype=np.int32)
    else:
        codes[:, 11:31] = 3 - stretch[:, ::-1]
        ae = np.full(n, 30, dtype=np.int32)
    return codes, ae


def _col(five_prime, s):
    """column of `codes` that holds base s of the stretch"""
    return 6 + s if five_prime else 30 - s


def _stretch_keys(stretch, d):
    return _pack(stretch[:, 2 - d:18 - d])


def _plant(keys_at, ds, rng):
    s = rng.integers(0, 4, (keys_at.size, 20), dtype=np.uint8)
    b = _bases16(keys_at)
    for d in DS:
        sel = ds == d
        s[sel, 2 - d:18 - d] = b[sel]
    return s


def _windows(pkg, codes, ae, five_prime):
    """the packing half of Parser.assignBarcode on the host -> BC_WINDOW_DTYPE records"""
    n, width = codes.shape
    W = 25 if five_prime else 24
    first = ae.astype(np.int64) - (1 if five_prime else 22)
    valid = (ae > 0) & (first >= 1) & (first + W - 1 <= width)
    win = np.take_along_axis(codes, np.clip(first - 1, 0, width - W)[:, None] + np.arange(W), 1).astype(np.uint64)
    is_n = win > 3
    rec = np.zeros(n, dtype=pkg.BC_WINDOW_DTYPE)
    rec["bases"] = np.where(valid, (np.where(is_n, U(0), win) << (np.arange(W - 1, -1, -1, dtype=np.uint64) * U(2))).sum(1), 0)
    rec["nmask"] = np.where(valid, (is_n.astype(np.uint64) << np.arange(W, dtype=np.uint64)).sum(1), 0)
    rec["flags"] = valid
    return rec


def _run(pkg, ctx, d_win, n, five_prime):
    d_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    ctx.bc_match_device(d_win[:n].contiguous(), d_out, n, max_ed=1, five_prime=five_prime)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(pkg.BC_RESULT_DTYPE).reshape(-1)


class Case:
    """windows on the device and the oracle's records for them (computed once per case)"""

    def __init__(self, pkg, sor, keys, codes, ae, five_prime):
        self.five_prime, self.n = five_prime, codes.shape[0]
        rec = _windows(pkg, codes, ae, five_prime)
        self.d_win = torch.from_numpy(rec.view(np.int64).reshape(-1, 2).copy()).cuda()
        self.st, self.exp = sor.assign_batch(sor.BarcodeSet(np.asarray(keys).astype(np.int64)), codes, ae, max_ed=1, five_prime=five_prime, n_threads=8)

    def check(self, pkg, ctx, monkeypatch, n=None):
        """default path == two-kernel path, byte for byte, == the oracle (found; the fields of an accepted barcode; n_matches of a valid window)"""
        n = self.n if n is None else n
        got = _run(pkg, ctx, self.d_win, n, self.five_prime)
        monkeypatch.setenv("SMI_BC1_TWO_KERNELS", "1")
        two = _run(pkg, ctx, self.d_win, n, self.five_prime)
        monkeypatch.delenv("SMI_BC1_TWO_KERNELS")
        assert (got.view(np.uint8) == two.view(np.uint8)).all(), (self.five_prime, n)
        st, exp = self.st[:n], self.exp[:n]
        assert (got["found"] == np.where(st < 0, st, exp["found"])).all(), (self.five_prime, n)
        assert (got["n_matches"][st < 0] == 0).all()
        sel = (st >= 0) & (exp["found"] == 1)
        for f in ("bc", "ed", "ed_sec", "offset", "ins_minus_del"):
            e = exp[f][sel].astype(np.int64) & (0xFFFFFFFF if f == "bc" else -1)
            assert (got[f][sel].astype(np.int64) == e).all(), (f, self.five_prime, n)
        assert (got["n_matches"][st >= 0] == exp["n_matches"][st >= 0]).all(), (self.five_prime, n)
        return got


def _key_list(synth, n, seed=171):
    return synth.make_whitelist(max(n, 16), seed=seed)[:n].numpy().astype(np.uint64)


def _passes_line_filter(nbh, stretch):
    """[n, 5]: the filter bit of nbl (a superset of the exact filters) of every read's window at each d of DS"""
    return np.stack([np.isin(nbl_cell(_stretch_keys(stretch, d), d), nbl_cell(nbh, d)) for d in DS], 1)


def _quiet_stretches(nbh, n, rng):
    """random stretches none of whose five windows passes the line filter"""
    s = rng.integers(0, 4, (4 * n + 64, 20), dtype=np.uint8)
    s = s[~_passes_line_filter(nbh, s).any(1)][:n]
    assert s.shape[0] == n
    return s


def _hit_reads(keys, n, rng):
    """read i carries member (7 i mod 169) of barcode i's neighbourhood at d = DS[i mod 5]; the last read of every size in SIZES the barcode itself at 0"""
    k_at = np.array([n1_member(keys[i:i + 1], (7 * i) % 169)[0] for i in range(n)], dtype=np.uint64)
    d_at = np.array([DS[i % 5] for i in range(n)])
    for m in SIZES:
        if m <= n:
            k_at[m - 1], d_at[m - 1] = keys[m - 1], 0
    return _plant(k_at, d_at, rng)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def test_sizes_invalid_and_n_windows(pkg, synth, sor, gpu_ctx, monkeypatch):
    """the last wave part full with a hit on the last read; invalid windows between valid ones; an N at the first, a middle and the last base of each
    offset's 16-mer (3': the emulated key, made a barcode of the list here, lies in another line of the filter; 5': an N-poisoned window is unusable)"""
    keys = _key_list(synth, 2_000)
    rng = np.random.default_rng(5)
    cases = {}
    extra = []
    for five_prime in (False, True):
        stretch = _hit_reads(keys, 193, rng)
        codes, ae = _records(stretch, five_prime, rng)
        # invalid windows between valid ones: a copy of the set with every third window not fitting its read
        codes_i, ae_i = codes.copy(), ae.copy()
        ae_i[1::3] = 1
        # N windows: barcode 300 + j planted at d, an N at base t of that 16-mer
        dn = np.repeat(np.array(DS), 3)
        tn = np.tile(np.array([0, 7, 15]), 5)
        sn = _plant(keys[300:315], dn, rng)
        codes_n, ae_n = _records(sn, five_prime, rng)
        codes_n[np.arange(15), [_col(five_prime, 2 - d + t) for d, t in zip(dn, tn)]] = 4
        if not five_prime:
            for r in range(15):  # the key the reference makes of the window with the N: in the list, it must be found
                w = codes_n[r, 7 + 6 + dn[r]:7 + 22 + dn[r]]
                extra.append(key_3p_with_n(np.where(w > 3, 0, w), w > 3))
        cases[five_prime] = [(codes, ae), (codes_i, ae_i), (np.concatenate([codes_n, codes[:49]]), np.concatenate([ae_n, ae[:49]]))]
    keys = np.unique(np.concatenate([keys, np.array(extra, dtype=np.uint64)]))
    gpu_ctx.set_barcode_set(keys, mode=0)
    for five_prime, (plain, invalid, with_n) in cases.items():
        c = Case(pkg, sor, keys, *plain, five_prime)
        for n in SIZES:
            got = c.check(pkg, gpu_ctx, monkeypatch, n)
            assert got["found"][n - 1] == 1 and got["ed"][n - 1] == 0 and got["offset"][n - 1] == 0, (five_prime, n)
        c = Case(pkg, sor, keys, *invalid, five_prime)
        got = c.check(pkg, gpu_ctx, monkeypatch)
        assert (got["found"][1::3] == -1).all() and (got["n_matches"][1::3] == 0).all() and (got["found"][0::3] >= 0).all()
        assert int((got["found"] == 1).sum()) > 64
        c = Case(pkg, sor, keys, *with_n, five_prime)
        got = c.check(pkg, gpu_ctx, monkeypatch)
        if five_prime:  # (the poisoned offset cannot match; a neighbouring offset may, through a deletion that drops the N's column)
            assert not ((got["found"][:15] == 1) & (got["ed"][:15] == 0)).any() and int((got["found"][:15] == 0).sum()) >= 10
        else:
            assert (got["found"][:15] == 1).all() and np.isin(got["bc"][:15].astype(np.uint64), np.array(extra, dtype=np.uint64)).all()


def _five_shifted(stretch):
    return np.concatenate([_stretch_keys(stretch, d) for d in DS])


def test_rounds_all_none_alternating(pkg, synth, sor, gpu_ctx, monkeypatch):
    """a wave in which every read passes all five offsets (320 pairs, five rounds: the list holds the five shifted 16-mers of every stretch), one in
    which none passes (no round: checked against a host model of the line filter), and one alternating reads of 0 and 5 pairs, so that the pairs of
    read 25 (numbers 60 .. 64) straddle the seam between the first two rounds"""
    rng = np.random.default_rng(6)
    filler = _key_list(synth, 1_000)
    full = rng.integers(0, 4, (64, 20), dtype=np.uint8)
    keys = np.unique(np.concatenate([filler, _five_shifted(full)]))
    nbh = neighbourhood(keys)
    assert _passes_line_filter(nbh, full).all()
    quiet = _quiet_stretches(nbh, 64, rng)
    alt = quiet.copy()
    alt[1::2] = full[1::2]
    gpu_ctx.set_barcode_set(keys, mode=0)
    for five_prime in (False, True):
        for name, stretch in (("all", full), ("none", quiet), ("alternating", alt)):
            codes, ae = _records(stretch, five_prime, rng)
            got = Case(pkg, sor, keys, codes, ae, five_prime).check(pkg, gpu_ctx, monkeypatch)
            hit = {"all": np.ones(64, bool), "none": np.zeros(64, bool), "alternating": np.arange(64) % 2 == 1}[name]
            assert (got["n_matches"][hit] >= 5).all() and (got["n_matches"][~hit] == 0).all(), (name, five_prime)
            assert (got["found"] == 0).all()  # (five barcodes at distance 0: ambiguous)


def _deletion_wave(five_prime, hit_pair, rng):
    """64 reads, the odd ones with five windows that ALL pass the filter and find an entry, none of them valid: window X of offset d is barcode w_d with a
    base inserted at position 5 and w_d's last base dropped, and w_d's last base is not the base the deletion appends -- but for pair `hit_pair` of the wave
    (read 2 (hit_pair // 5) + 1, offset OFFS[hit_pair % 5]), whose barcode ends in the appended base.  -> stretches, column-26 bases (5': the base behind
    the stretch), the list, the hit's (read, barcode, record-side offset)"""
    q = 5
    stretch = rng.integers(0, 4, (64, 20), dtype=np.uint8)
    behind = rng.integers(0, 4, 64, dtype=np.uint8)
    keys, hit = [], None
    for k in range(32):
        r = 2 * k + 1
        for pair_q, o in enumerate(OFFS):
            d = -o if five_prime else o
            x = stretch[r, 2 - d:18 - d]
            if five_prime:
                db = behind[r] if 18 - d == 20 else stretch[r, 18 - d]
            else:
                db = x[15]
            is_hit = 5 * k + pair_q == hit_pair
            w = np.concatenate([x[:q], x[q + 1:], [db if is_hit else (db + 1) & 3]])
            keys.append(_pack(w))
            if is_hit:
                hit = (r, int(_pack(w)), o)
    return stretch, behind, np.array(keys, dtype=np.uint64), hit


@pytest.mark.parametrize("hit_pair", [63, 64, 65])
def test_single_hit_at_the_round_seam(pkg, synth, sor, gpu_ctx, monkeypatch, hit_pair):
    """the alternating wave (160 pairs, all looked up) with the single hit at the last pair of the first round, the first and the second of the second"""
    for five_prime in (False, True):
        for attempt in range(20):  # (random stretches: now and then a window is a chance neighbour of another barcode; the ORACLE says when none is)
            rng = np.random.default_rng(700 + 40 * attempt + 2 * hit_pair + five_prime)
            stretch, behind, planted, (r_hit, bc_hit, o_hit) = _deletion_wave(five_prime, hit_pair, rng)
            keys = np.unique(np.concatenate([_key_list(synth, 1_000), planted]))
            nbh = neighbourhood(keys)
            stretch[0::2] = _quiet_stretches(nbh, 32, rng)
            codes, ae = _records(stretch, five_prime, rng)
            if five_prime:
                codes[:, 26] = behind
            case = Case(pkg, sor, keys, codes, ae, five_prime)
            if int((case.exp["n_matches"] > 0).sum()) == 1:
                break
        else:
            raise AssertionError("no wave with a single hit in 20 draws")
        passes = _passes_line_filter(nbh, stretch)
        assert passes[1::2].all() and not passes[0::2].any()
        gpu_ctx.set_barcode_set(keys, mode=0)
        got = case.check(pkg, gpu_ctx, monkeypatch)
        others = np.arange(64) != r_hit
        assert (got["found"][others] == 0).all() and (got["n_matches"][others] == 0).all(), five_prime
        h = got[r_hit]
        assert (h["found"], h["bc"], h["ed"], h["offset"], h["ins_minus_del"], h["n_matches"]) == (1, bc_hit, 1, o_hit, 1, 1), five_prime


def test_second_bucket(pkg, synth, sor, gpu_ctx, monkeypatch):
    """look-ups that walk into a second bucket, by construction: a bucket that nine or more (barcode, step) pairs of the list call home is full and has
    sent at least one entry on to the next one, so every look-up of a sequence of that bucket reads both, and one of them finds its entry only there"""
    keys = _key_list(synth, 2_000)
    gpu_ctx.set_barcode_set(keys, mode=0)
    stats = gpu_ctx.set_stats(digests=True)
    cap = stats["nt_slots"]
    assert cap % 8 == 0 and stats["nt_entries"] == 169 * keys.size
    members = np.concatenate([n1_member(keys, s) for s in range(169)])
    home = nt_bucket(members, cap)
    buckets, counts = np.unique(home, return_counts=True)
    x = np.unique(members[np.isin(home, buckets[counts >= 9])])
    assert x.size >= 64
    x = x[:512]
    rng = np.random.default_rng(8)
    for five_prime in (False, True):
        codes, ae = _records(_plant(x, np.zeros(x.size, dtype=np.int64), rng), five_prime, rng)
        got = Case(pkg, sor, keys, codes, ae, five_prime).check(pkg, gpu_ctx, monkeypatch)
        assert int((got["n_matches"] > 0).sum()) > x.size // 2  # (a deletion's or the last insertion's neighbour may be no match for this read)


def test_pick_rules(pkg, synth, sor, gpu_ctx, monkeypatch):
    """the pick's rules through the new path: exact at offset 0 beside a level-1 hit at offset -1; two different barcodes at the same distance; a deletion
    whose appended base is / is not the read's next base; the insertion behind position 14 of a window ending / not ending in A"""
    for five_prime in (False, True):
        rng = np.random.default_rng(90 + five_prime)
        sgn = -1 if five_prime else 1   # d of record-side offset o
        s = rng.integers(0, 4, (6, 20), dtype=np.uint8)
        behind = rng.integers(0, 4, 6, dtype=np.uint8)
        sub8 = U(1 << (30 - 2 * 8))
        # 0: exact at offset 0, one substitution away from another barcode at offset -1
        a0 = _stretch_keys(s[0:1], 0)[0]
        b0 = _stretch_keys(s[0:1], sgn * -1)[0] ^ U(1 << 30)  # (at position 0: in front of the deletion of position 0, which in a 5' read leads back to a0)
        # 1: one substitution from one barcode at offset 0 and from another at offset 1
        a1 = _stretch_keys(s[1:2], 0)[0] ^ sub8
        b1 = _stretch_keys(s[1:2], sgn * 1)[0] ^ sub8
        # 2, 3: window = barcode with a base inserted at 5, last base dropped; the barcode's last base is (2) / is not (3) what the deletion appends
        dels = []
        for r in (2, 3):
            x = s[r, 2:18]
            db = (s[r, 18] if five_prime else x[15])
            dels.append(_pack(np.concatenate([x[:5], x[6:], [db if r == 2 else (db + 1) & 3]])))
        # 4, 5: window = barcode with its last base (C) replaced by A (4: the insertion behind position 14 comes first) / by G (5: only the substitution)
        s[4, 17], s[5, 17] = 0, 1
        ins = [(_stretch_keys(s[r:r + 1], 0)[0] & ~U(3)) | U(2) for r in (4, 5)]
        keys = np.unique(np.concatenate([_key_list(synth, 1_000), np.array([a0, b0, a1, b1] + dels + ins, dtype=np.uint64)]))
        codes, ae = _records(s, five_prime, rng)
        if five_prime:
            codes[:, 26] = behind
        gpu_ctx.set_barcode_set(keys, mode=0)
        got = Case(pkg, sor, keys, codes, ae, five_prime).check(pkg, gpu_ctx, monkeypatch)

        def rec(i):
            return tuple(int(got[f][i]) for f in ("found", "bc", "ed", "ed_sec", "offset", "ins_minus_del", "n_matches"))

        assert rec(0)[:6] == (1, int(a0), 0, 1, 0, 0) and rec(0)[6] >= 2, five_prime
        assert rec(1)[0] == 0 and rec(1)[6] == 2, five_prime
        assert rec(2) == (1, int(dels[0]), 1, 2147483647, 0, 1, 1), five_prime
        assert rec(3)[0] == 0 and rec(3)[6] == 0, five_prime
        assert rec(4) == (1, int(ins[0]), 1, 2147483647, 0, -1, 1), five_prime
        assert rec(5) == (1, int(ins[1]), 1, 2147483647, 0, 0, 1), five_prime


def test_random_windows(pkg, synth, gpu_ctx, monkeypatch):
    """100,000 windows drawn from a 50,000-key list with 0, 1 or 2 steps of the enumeration applied, at a random offset: default path == two-kernel path"""
    keys = _key_list(synth, 50_000, seed=172)
    gpu_ctx.set_barcode_set(keys, mode=0)
    n = 100_000
    for five_prime in (False, True):
        rng = np.random.default_rng(10 + five_prime)
        k = keys[rng.integers(0, keys.size, n)]
        n_mut = rng.integers(0, 3, n)
        for turn in (1, 2):
            slot = rng.integers(0, 168, n)
            for sl in range(168):
                sel = (slot == sl) & (n_mut >= turn)
                k[sel] = n1_member(k[sel], sl)
        stretch = _plant(k, np.array(DS)[rng.integers(0, 5, n)], rng)
        codes, ae = _records(stretch, five_prime, rng)
        d_win = torch.from_numpy(_windows(pkg, codes, ae, five_prime).view(np.int64).reshape(-1, 2).copy()).cuda()
        got = _run(pkg, gpu_ctx, d_win, n, five_prime)
        monkeypatch.setenv("SMI_BC1_TWO_KERNELS", "1")
        two = _run(pkg, gpu_ctx, d_win, n, five_prime)
        monkeypatch.delenv("SMI_BC1_TWO_KERNELS")
        assert (got.view(np.uint8) == two.view(np.uint8)).all(), five_prime
        assert int((got["found"] == 1).sum()) > n // 3 and int((got["ed"][got["found"] == 1] == 1).sum()) > n // 10
