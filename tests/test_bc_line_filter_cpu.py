"""K-BC1's line filter `nbl` (smi_bc.hip): a numpy restatement of nb5_bit_index and nbl_bit_index, and the properties the kernel relies on --
every (offset, key) of one read lands in ONE 32-word row (an aligned 128-byte line), offsets 0 and +-1 keep nb5's bits one to one, offsets +-2
put nb5's words j and j + 4 onto word j & 3 and nothing else.  No GPU."""
import numpy as np
import pytest

DS = (-2, -1, 0, 1, 2)
BASE = {-2: 0, -1: 4, 0: 12, 1: 20, 2: 28}
MASK = {-2: 3, -1: 7, 0: 7, 1: 7, 2: 3}
WORDS = {-2: 4, -1: 8, 0: 8, 1: 8, 2: 4}


def _core_flank(key, d):
    key = np.asarray(key, dtype=np.uint64)
    sh = 2 * (2 - d)
    core = (key >> np.uint64(sh)) & np.uint64(0xFFFFFF)
    low = np.uint64((1 << sh) - 1)
    flank = ((key >> np.uint64(24)) & ~low & np.uint64(0xFF)) | (key & low)
    return core, flank


def nb5_index(key, d):
    core, flank = _core_flank(key, d)
    return core * np.uint64(40) + np.uint64((d + 2) * 8) + (flank >> np.uint64(5)), flank & np.uint64(31)


def nbl_index(key, d):
    core, flank = _core_flank(key, d)
    # (a sum: the bases 4, 12 and 20 are no multiples of eight, so ORing a word number 0 .. 7 onto them would collide)
    return (core << np.uint64(5)) + np.uint64(BASE[d]) + ((flank >> np.uint64(5)) & np.uint64(MASK[d])), flank & np.uint64(31)


def _keys():
    rng = np.random.default_rng(2024)
    rnd = rng.integers(0, 1 << 32, 20_000, dtype=np.uint64)
    structured = [0, 0xFFFFFFFF, 0x55555555, 0xAAAAAAAA, 0x00FFFF00, 0xFF0000FF, 1, 1 << 31]
    # pairs that differ only in the flank bit the fold drops: bit 7 of the flank = key bit 7 at d = -2 (the flank is the last four bases), key bit 31 at
    # d = +2 (the first four)
    pairs = []
    for k in list(rnd[:500]) + structured:
        pairs += [int(k) ^ 0x80, int(k) ^ 0x80000000, int(k) ^ 0x80000080]
    return np.unique(np.concatenate([rnd, np.array(structured + pairs, dtype=np.uint64)]))


def test_layout_constants():
    """4 / 8 / 8 / 8 / 4 words at bases 0 / 4 / 12 / 20 / 28: the five blocks tile the 32 words of a row exactly"""
    covered = []
    for d in DS:
        assert MASK[d] == WORDS[d] - 1
        covered += list(range(BASE[d], BASE[d] + WORDS[d]))
    assert covered == list(range(32))
    # 2^24 rows of 32 words: 2 GiB, the largest word index fits 32 bits
    w, _ = nbl_index(np.array([0xFFFFFFFF], dtype=np.uint64), 2)
    assert int(w[0]) < (1 << 29) and (1 << 24) * 32 * 4 == 1 << 31


@pytest.mark.parametrize("d", DS)
def test_same_core_row_and_block(d):
    keys = _keys()
    w5, b5 = nb5_index(keys, d)
    wl, bl = nbl_index(keys, d)
    assert ((wl >> np.uint64(5)) == w5 // np.uint64(40)).all()          # the same core row
    assert (bl == b5).all()                                              # the same bit of the word
    local = wl & np.uint64(31)
    assert ((local >= BASE[d]) & (local < BASE[d] + WORDS[d])).all()     # inside the block of this offset
    j5 = w5 % np.uint64(40) - np.uint64((d + 2) * 8)
    assert (j5 < 8).all() and (local - np.uint64(BASE[d]) == (j5 & np.uint64(MASK[d]))).all()


def test_five_windows_of_a_stretch_share_one_row():
    """a read's five windows are one 20-base stretch cut at five places: the key of offset d is bases 2 - d .. 17 - d of it, and all five (word, bit)
    positions lie in the 32 words of the row of the 12 middle bases"""
    rng = np.random.default_rng(7)
    stretch = rng.integers(0, 4, (5000, 20), dtype=np.uint64)
    stretch[0] = 0
    stretch[1] = 3
    stretch[2, :4] = 3   # a stretch whose flanks are all T around an all-A core
    stretch[2, 4:16] = 0
    stretch[2, 16:] = 3
    shifts = np.arange(15, -1, -1, dtype=np.uint64) * np.uint64(2)
    core = (stretch[:, 4:16] << (np.arange(11, -1, -1, dtype=np.uint64) * np.uint64(2))).sum(1)
    seen = []
    for d in DS:
        key = (stretch[:, 2 - d:18 - d] << shifts).sum(1)
        wl, _ = nbl_index(key, d)
        assert ((wl >> np.uint64(5)) == core).all()
        assert (wl * np.uint64(4) // np.uint64(128) == core).all()      # one aligned 128-byte line per core
        seen.append(wl & np.uint64(31))
    seen = np.stack(seen, 1)
    assert (np.sort(seen, 1) == seen).all() and (np.diff(seen.astype(np.int64), axis=1) > 0).all()  # five different words, in offset order


@pytest.mark.parametrize("core", [0, 0xFFFFFF, 0x123456, 0xABCDEF])
def test_exact_offsets_one_to_one_outer_offsets_two_to_one(core):
    """all 256 flanks of one core: offsets 0 and +-1 keep 256 distinct bits, in nb5's order; offsets +-2 map exactly the two nb5 positions
    (j, bit) and (j + 4, bit) onto (j & 3, bit)"""
    for d in DS:
        sh = 2 * (2 - d)
        flank = np.arange(256, dtype=np.uint64)
        low = np.uint64((1 << sh) - 1)
        key = ((flank & ~low) << np.uint64(24)) | (np.uint64(core) << np.uint64(sh)) | (flank & low)
        c, f = _core_flank(key, d)
        assert (c == core).all() and (f == flank).all()
        w5, b5 = nb5_index(key, d)
        wl, bl = nbl_index(key, d)
        p5 = (w5 - np.uint64(core * 40 + (d + 2) * 8)) * np.uint64(32) + b5      # position in nb5's block: the flank itself
        pl = (wl - np.uint64(core * 32 + BASE[d])) * np.uint64(32) + bl
        assert (p5 == flank).all()
        if d in (-1, 0, 1):
            assert (pl == p5).all() and np.unique(pl).size == 256
        else:
            assert (pl == (p5 & np.uint64(127))).all()
            u, cnt = np.unique(pl, return_counts=True)
            assert u.size == 128 and (cnt == 2).all()
            for x in (0, 31, 32, 127):
                assert sorted(int(v) for v in p5[pl == x]) == [x, x + 128]       # words j and j + 4, the same bit, nothing else


def test_fold_of_rows_is_the_index_function():
    """the build folds nb5 row by row (words 4 .. 7 of the first and last block ORed onto words 0 .. 3); the probe uses nbl_bit_index: both name the
    same bit for every (key, d)"""
    keys = _keys()
    for d in DS:
        w5, b5 = nb5_index(keys, d)
        row, j = w5 // np.uint64(40), w5 % np.uint64(40)
        folded = np.where(j < 8, j & np.uint64(3), np.where(j < 32, j - np.uint64(4), np.uint64(28) + ((j - np.uint64(32)) & np.uint64(3))))
        wl, bl = nbl_index(keys, d)
        assert (row * np.uint64(32) + folded == wl).all() and (bl == b5).all()
