"""The catalogue of tests/test_scan_bits_gpu.py, proved without the device.  K-SCAN's phase A computes its masks on 32-bit words in three-input
operations (smi_scan.hip "Three-input forms"): the polyT finder's bit-sliced counts and entry mask, the walk back's mask on the two halves of a 64-bit
window, the smear of the isolated TSO candidates on three words.  tools/scan_finder_model.py (front_words, back_mask_words) and tools/scan_gate_model.py
(isolated_words) restate those operations word for word; here they are held against the loops (masks_of, the oracle's find_polyt, isolated) on ends
whose deciding bits lie on the words' seams, and on random masks.

polyT ends (all C, T's planted; the complete adapter at scan position 3 where the run leaves room for it, so that a record shows where the polyT ends):
  seam_P        thirteen T's from 0-based position P on: the entry at P passes with exactly 12 T's among its fifteen bases [P + 1, P + 16), no other
                position does.  P = 18 .. 33, 50 .. 65, 82 .. 97, 114 .. 129: a 32-bit seam at every place of the sixteen bases, and just below them
  seam_P_eleven one T less: no entry at all (these ride along in the batches as the other reads)
  entry_at_0, entry_at_149, entry_at_150 (none: the window ends at 149)
  entry_twelve_of_15 / entry_eleven_of_15     the non-T's spread over the fifteen bases, across the seam at 64
  probe_ten / probe_nine                       the stride-20 probe of the extension meets exactly 10 / 9 T's, across the seam at 96
  first_five_three / first_five_two            3 / 2 T's among the entry's first five bases, which straddle the seam at 32
  back_seam_5 .. back_seam_8                   the walk back ends 5 .. 8 positions below start + 14: the five bases that decide it straddle the two
                                               halves of the 64-bit window the mask is built on (the window begins 40 below start + 14)
TSO ends: two candidates at distance 26 and 27 -- a whole TSO and five bases of it on the diagonal ("five": gated, and min Levenshtein over the
leading gaps > 5, so the bound drops it once it is isolated) in both orders -- across scan positions 63 / 64 and 64 / 65 (bits 62 .. 64 of the mask),
ending at position 90 and starting at position 1.  The pre-filter is exact: whether a candidate is aligned or dropped by the bound, a record never
shows it, and no gated 16-mer has the 31.5 errors a jump of 26 takes -- so at these distances a smear that is off by one position could not change a
record.  The smear's arithmetic is therefore proved here, on every pair of positions and on random masks, against the loop; the GPU test holds the
kernels' records on these ends to the oracle and to the generic kernels, which align every candidate."""
import random

import numpy as np
import pytest

from test_scan_finder_cpu import WINDOW, both, c_end, codes_of, fm
from test_scan_gpu import AD
from test_scan_lanes_gpu import F_A3, F_BOTH, F_T5, TSO, _batch, _codes, _put, gm

SEAM_STARTS = [p for lo in (18, 50, 82, 114) for p in range(lo, lo + 16)]


def t_end(tpos):
    """an all-C end with T at the 0-based positions tpos; the complete adapter at scan position 3 where the first T leaves room for it"""
    tpos = sorted(tpos)
    e = c_end()
    if tpos[0] >= 27:
        _put(e, 3, AD[1])
    for p in tpos:
        e[p] = "T"
    return e


def _spread(p, more=()):
    """T at p; among the fifteen bases behind it everything but p + 5, p + 10, p + 15 (and `more`) is a T"""
    return t_end([p] + [q for q in range(p + 1, p + 16) if q not in (p + 5, p + 10, p + 15) + tuple(more)])


def _probe(a, holes):
    """a run of 36 T's from a on with non-T's at `holes`: the stride-20 probe at a + 20 counts the T's of [a + 21, a + 36)"""
    return t_end([q for q in range(a, a + 36) if q not in holes])


def _back(k, a=60, b=110):
    """a run a .. b - 2 k, then k times `C T`: the probes carry `start` to b - 10 - k, and the last position that passes `back` lies 4 + k below start + 14"""
    return t_end(list(range(a, b - 2 * k + 1)) + [b - 2 * j for j in range(k)])


# name -> (end, first: the 0-based entry position, -1 = no polyT)
POLYT, RIDERS = {}, {}
for _p in SEAM_STARTS:
    POLYT[f"seam_{_p:03d}"] = (t_end(range(_p, _p + 13)), _p)
    RIDERS[f"seam_{_p:03d}_eleven"] = (t_end(range(_p, _p + 12)), -1)
POLYT["entry_at_0"] = (t_end(range(0, 13)), 0)
POLYT["entry_at_149"] = (t_end(range(149, 162)), 149)
RIDERS["entry_at_150"] = (t_end(range(150, 163)), -1)
POLYT["entry_twelve_of_15"] = (_spread(60), 60)
POLYT["entry_eleven_of_15"] = (_spread(60, (73,)), -1)
PROBE_AT, PROBE_HOLES = 65, (87, 90, 93, 96, 99)
POLYT["probe_ten"] = (_probe(PROBE_AT, PROBE_HOLES), PROBE_AT)
POLYT["probe_nine"] = (_probe(PROBE_AT, PROBE_HOLES + (97,)), PROBE_AT)
POLYT["first_five_three"] = (t_end([30, 33, 34] + list(range(35, 45))), 30)
POLYT["first_five_two"] = (t_end([30, 34] + list(range(35, 46))), -1)
for _k in (1, 2, 3, 4):
    POLYT[f"back_seam_{4 + _k}"] = (_back(_k), 60)
ALL_POLYT = {**POLYT, **RIDERS}


def t_bits(end):
    return fm.masks_of(codes_of(end))[0]


def end1_of(end):
    """1-based end of the polyT as the loops give it, or 0"""
    T, G, first = fm.masks_of(codes_of(end))
    return fm.tail_loops(T, G, first, WINDOW)[2] if first >= 0 else 0


@pytest.mark.parametrize("name", sorted(ALL_POLYT))
def test_polyt_catalogue(sor, name):
    end, want = ALL_POLYT[name]
    codes = codes_of(end)
    T, G, first = fm.masks_of(codes)
    assert first == want
    assert fm.front_words(T, WINDOW) == (G, first)              # the kernel's words and three-input forms say what the loop over positions says
    got = sor.find_polyt(codes[:WINDOW + 25])                   # the loop finder
    if first < 0:
        assert got is None
        return
    (start, endpos, end1), loops, _ = both(T, G, first)         # the tail as loops == the tail as masks
    assert (int(got[0]), int(got[1])) == (first + 1, end1)
    n15 = fm.popc((T >> (first + 1)) & 0x7FFF)
    if name.startswith("seam_") or name in ("entry_at_0", "entry_at_149", "entry_twelve_of_15"):
        assert n15 == 12                                         # exactly at the threshold
        if name.startswith("seam_"):
            assert any(first - 2 <= s <= first + 15 for s in (32, 64, 96, 128))   # a seam inside the sixteen bases, or just below them
    if name.startswith("back_seam_"):
        k = int(name[-1])
        assert loops["back"] == k and 5 <= k <= 8                # e in [start + 14 - 8, start + 14 - 5]: e - 4 .. e straddles bits 31 | 32 of the window


def test_thresholds_are_exact():
    """the pairs differ in one base and sit on either side of a threshold"""
    T12, T11 = t_bits(POLYT["entry_twelve_of_15"][0]), t_bits(POLYT["entry_eleven_of_15"][0])
    assert fm.popc((T12 >> 61) & 0x7FFF) == 12 and fm.popc((T11 >> 61) & 0x7FFF) == 11 and fm.popc(T12 ^ T11) == 1
    assert 61 // 32 != 75 // 32
    for p in SEAM_STARTS:
        assert fm.popc((t_bits(RIDERS[f"seam_{p:03d}_eleven"][0]) >> (p + 1)) & 0x7FFF) == 11
    T10, T9 = t_bits(POLYT["probe_ten"][0]), t_bits(POLYT["probe_nine"][0])
    a = PROBE_AT
    assert fm.popc((T10 >> (a + 21)) & 0x7FFF) == 10 and fm.popc((T9 >> (a + 21)) & 0x7FFF) == 9 and fm.popc(T10 ^ T9) == 1
    assert (a + 21) // 32 != (a + 35) // 32
    G10, G9 = fm.masks_of(codes_of(POLYT["probe_ten"][0]))[1], fm.masks_of(codes_of(POLYT["probe_nine"][0]))[1]
    assert (G10 >> (a + 20)) & 1 and not (G9 >> (a + 20)) & 1
    assert end1_of(POLYT["probe_ten"][0]) != end1_of(POLYT["probe_nine"][0])      # the probe decides where the polyT ends: a record shows it
    T3, T2 = t_bits(POLYT["first_five_three"][0]), t_bits(POLYT["first_five_two"][0])
    assert fm.popc((T3 >> 30) & 31) == 3 and fm.popc((T2 >> 30) & 31) == 2
    assert fm.popc((T3 >> 31) & 0x7FFF) == 12 and fm.popc((T2 >> 31) & 0x7FFF) == 12   # the fifteen-count passes in both: the five bases decide
    assert len({end1_of(POLYT[f"back_seam_{k}"][0]) for k in (5, 6, 7, 8)}) == 4


@pytest.mark.parametrize("seed", range(4))
def test_front_words_on_random_masks(seed):
    """the bit-sliced front == the loop over positions on any exact-T mask, at the shipped window and at windows that end on and next to a word"""
    rng = random.Random(9100 + seed)
    for i in range(1500):
        T = rng.getrandbits(208)
        for _ in range(i % 4):
            T |= rng.getrandbits(208)                          # 50 % .. 94 % T: entries and probes at every density
        if i % 3 == 0:
            T &= ~(((1 << rng.randrange(10, 60)) - 1) << rng.randrange(0, 160))
        window = (150, 149, 129, 128, 97, 160, 1, 33)[i % 8]
        codes = np.array([8 if (T >> p) & 1 else 4 for p in range(208)], dtype=np.uint8)
        _, G, first = fm.masks_of(codes, window)
        assert fm.front_words(T, window) == (G, first), (hex(T), window)


def test_back_mask_words():
    rng = random.Random(9200)
    for i in range(20000):
        w = rng.getrandbits(64) | (rng.getrandbits(64) if i % 2 else 0)
        l1, l2, l3, l4 = ((w << s) & fm.M64 for s in (1, 2, 3, 4))
        assert fm.back_mask_words(w) == w & l1 & ((l2 & l3) | (l4 & (l2 ^ l3)))


# ---- the TSO pairs ---------------------------------------------------------------------------------------------------------------------------
FIVE = TSO[:5]
# name -> ((kind, scan position), (kind, scan position)); "far": distance 27, the first of the pair is isolated; "near": 26, it is not
TSO_PAIRS = {}
for _tag, _a26, _a27, _b in (("across_63_64", 38, 37, 64), ("across_64_65", 39, 38, 65), ("ending_at_90", 64, 63, 90)):
    for _dist, _a in (("near", _a26), ("far", _a27)):
        TSO_PAIRS[f"{_tag}_{_dist}_five_first"] = (("five", _a), ("tso", _b))
        TSO_PAIRS[f"{_tag}_{_dist}_tso_first"] = (("tso", _a), ("five", _b))
for _dist, _b in (("near", 27), ("far", 28)):
    TSO_PAIRS[f"starting_at_1_{_dist}_five_first"] = (("five", 1), ("tso", _b))
    TSO_PAIRS[f"starting_at_1_{_dist}_tso_first"] = (("tso", 1), ("five", _b))


def tso_pair_end(name):
    e = c_end()
    for kind, p in TSO_PAIRS[name]:
        _put(e, p, TSO if kind == "tso" else FIVE)
    return e


def five_end(p):
    e = c_end()
    _put(e, p, FIVE)
    return e


def _lev(a, b):
    d = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        nd = [i]
        for j, cb in enumerate(b, 1):
            nd.append(min(d[j] + 1, nd[j - 1] + 1, d[j - 1] + (ca != cb)))
        d = nd
    return d[-1]


def tso_bound(sl):
    """smi_nw.h myers_bound_tso16(V, 5): min over s <= 5 leading template gaps of Levenshtein(TSO, slice[s ..])"""
    return min(_lev(TSO, sl[s:]) for s in range(6))


def tso_masks(end):
    tm = gm.gate_masks(_codes([(end, c_end())])[:1], TSO, gm.TSO_WINDOW)
    return tm, gm.isolated(tm)


@pytest.mark.parametrize("name", sorted(TSO_PAIRS))
def test_tso_pairs(sor, name):
    from test_scan_lazy_cpu import _tso_rec

    (k1, p1), (k2, p2) = TSO_PAIRS[name]
    end = tso_pair_end(name)
    tm, iso = tso_masks(end)
    assert (np.nonzero(tm[0])[0] + 1).tolist() == [p1, p2]                # the two planted candidates and no other
    assert p2 - p1 == (26 if "_near_" in name else 27)
    assert bool(iso[0, p1 - 1]) == ("_far_" in name) and bool(iso[0, p2 - 1])  # the second is always isolated, the first at distance 27 only
    assert (gm.isolated_words(tm) == iso).all()
    text = "".join(end)
    for kind, p in TSO_PAIRS[name]:
        b = tso_bound(text[p - 1:p + 15])
        assert (b > 5) == (kind == "five"), (kind, p, b)                  # the bound drops the five bases wherever they are isolated, never the TSO
    five_p, tso_p = (p1, p2) if k1 == "five" else (p2, p1)
    assert bool(iso[0, five_p - 1]) == (five_p == p2 or "_far_" in name)
    got = _tso_rec(sor, end, c_end())                                     # the oracle alone: the whole TSO is found, on the head
    assert got[0] != 0 and got[1] == 0
    alone = c_end()
    _put(alone, tso_p, TSO)
    assert _tso_rec(sor, alone, c_end()) == got                           # ... exactly as without the five bases: dropped or aligned, they change nothing


def test_smear_words_on_every_pair_and_on_random_masks():
    """isolated as the kernel's three words compute it == the loop over the next 26 positions"""
    P = gm.TSO_WINDOW
    rows = []
    for a in range(P):
        for d in (1, 2, 3, 4, 9, 10, 17, 18, 25, 26, 27, 28, 31, 32, 33, 58, 63, 64, 65):
            if a + d < P:
                m = np.zeros(P, dtype=bool)
                m[a] = m[a + d] = True
                rows.append(m)
    rng = np.random.default_rng(9300)
    for dens in (0.01, 0.03, 0.1, 0.3):
        rows.extend(rng.random((300, P)) < dens)
    mask = np.array(rows)
    assert (gm.isolated_words(mask) == gm.isolated(mask)).all()
    iso = gm.isolated(mask)
    assert iso.any() and (mask & ~iso).any()


# ---- the batches of the GPU test, and what the oracle says about them ----------------------------------------------------------------------------
NAMES, RIDER_NAMES = sorted(POLYT), sorted(RIDERS)
OTHERS = RIDER_NAMES + NAMES
SIZES = (1, 33, 65)


def polyt_batch(n, name, k):
    """n reads: `name` on read 0's head (lane 0), on read 31's tail (lane 63) and on the last read's tail; the other reads carry the rest of the catalogue,
    riders included, on alternating sides -> [(head, tail)], [(name, side)]"""
    ends, where = [], []
    for i in range(n):
        nm, side = OTHERS[(11 * k + i) % len(OTHERS)], i % 2
        if i == 0:
            nm, side = name, 0
        elif i == 31 or i == n - 1:
            nm, side = name, 1
        own = list(ALL_POLYT[nm][0])
        ends.append((own, c_end()) if side == 0 else (c_end(), own))
        where.append((nm, side))
    return ends, where


def check_polyt_records(exp, offs, where):
    """the oracle's pass-2 records of a polyt_batch: the flag of the side that carries a polyT, and its end wherever the adapter stands in front of it"""
    fl = exp["flags"].astype(np.int64)
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    pe = np.where(exp["polya_start"] != 0, lens - exp["polya_start"] + 1, 0)
    for i, (nm, side) in enumerate(where):
        end, first = ALL_POLYT[nm]
        want = 0 if first < 0 else (F_A3 if side else F_T5)
        assert fl[i] & (F_T5 | F_A3 | F_BOTH) == want, (i, nm, side)
        if first >= 27:
            assert pe[i] == end1_of(end), (i, nm, pe[i])


def tso_batch(n, name):
    """n reads: the pair on read 0's head, on read 31's tail and on the last read's tail, five bases alone on the other end of those reads; every other
    read carries a whole TSO on one end and five bases on the other -- a wave of 64 ends holds more than 64 candidates, of which all but a few are isolated"""
    from test_scan_lazy_cpu import whole

    ends, where = [], {}
    for i in range(n):
        if i == 0:
            ends.append((tso_pair_end(name), five_end(40)))
            where[i] = 0
        elif i == 31 or i == n - 1:
            ends.append((five_end(40), tso_pair_end(name)))
            where[i] = 1
        else:
            ends.append((whole(i), five_end(20 + i)) if i % 2 else (five_end(20 + i), whole(i)))
    return ends, where


def check_tso_records(exp, where):
    t = np.stack([exp["tso_start"], exp["tso_end"]], 1) != 0
    for i in range(t.shape[0]):
        side = where.get(i, 0 if i % 2 else 1)                 # the end that carries a whole TSO
        assert t[i].tolist() == [side == 0, side == 1], (i, t[i])


def test_what_the_oracle_says_about_the_batches(sor):
    """the GPU test's own assertions, held against the oracle alone"""
    for n in SIZES:
        for k, name in enumerate(NAMES[::9] + ["entry_at_0", "probe_nine"]):
            ends, where = polyt_batch(n, name, k)
            ra, qa, offs = _batch(ends, np.random.default_rng(9400 + n + k))
            check_polyt_records(sor.scan_batch_3p(ra, qa, offs, AD[2], n_threads=4)[1], offs, where)
        for name in sorted(TSO_PAIRS)[::3]:
            ends, where = tso_batch(n, name)
            ra, qa, offs = _batch(ends, np.random.default_rng(9500 + n))
            check_tso_records(sor.scan_batch_3p(ra, qa, offs, AD[2], n_threads=4)[1], where)


@pytest.mark.parametrize("name", sorted(TSO_PAIRS))
def test_the_prefilter_runs_in_the_first_wave(name):
    """the shipped kernel smears and drops only where that saves a round of 64 alignments: the first wave of the batches of 33 and 65 reads is built so"""
    ends, _ = tso_batch(33, name)
    tm = gm.gate_masks(_codes(ends[:32]), TSO, gm.TSO_WINDOW)
    total, n_iso = int(tm.sum()), int(gm.isolated(tm).sum())
    assert total > 64 and (total + 63) // 64 > (total - n_iso + 63) // 64
    assert (gm.isolated_words(tm) == gm.isolated(tm)).all()
