"""The tail of K-SCAN's bit-parallel polyT finder (smi_scan.hip find_polyt_bits behind `first`: extension, walk back, forward steps) as the loops of
the reference and as the kernel's mask operations, both restated over integer masks in tools/scan_finder_model.py: equal `start`, `endpos` and `end1`
on seeded random masks and on structured ones.  What can be planted as bases is planted on the all-C background of the other scan tests (PLANTS:
tests/test_scan_finder_gpu.py runs the same ends through the kernels), and the oracle's find_polyt proves what each plant is.  Three of the
structured cases cannot be bases: an entry position needs twelve T's among the fifteen bases behind it, and so does every probe that moved `start` ten;
such an end always has a `back` position a few bases below start + 14 -- no result 4, no walk back of 36 positions, no walk down to positions 4 and 5.
Those are masks only, where the two tails must agree on ANY pair of masks.
Also here: two adapter ties whose keys (smi_nw.h nw_end_errors) differ in one of the two counts alone, proved by the oracle."""
import os
import random
import sys

import numpy as np
import pytest

from test_scan_gpu import AD
from test_scan_lanes_gpu import E, _put

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import scan_finder_model as fm  # noqa: E402

WINDOW = 150
CODE = {"A": 1, "G": 2, "C": 4, "T": 8, "N": 15}
HOLE = (1, 4, 7, 10, 13, 15)     # non-T bases at h + these offsets inside a T run: nine T's in [h + 1, h + 16), ten in both neighbours' windows


def c_end():
    return ["C"] * E


def run_end(a, b, holes=(), n_at=()):
    """an all-C end with T at the 0-based positions a .. b; holes: probe positions h that get exactly nine T's behind them; n_at: positions set to N.
    Where there is room in front of the run, the complete adapter stands at scan position 3: the record of a read shows where its polyT ends only
    when the end has an adapter candidate"""
    e = c_end()
    if a >= 27:
        _put(e, 3, AD[1])
    _put(e, a + 1, "T" * (min(b, E - 1) - a + 1))
    for h in holes:
        for d in HOLE:
            e[h + d] = "C"
    for p in n_at:
        e[p] = "N"
    return e


def codes_of(end):
    return np.array([CODE[c] for c in end], dtype=np.uint8)


# name -> (the end, what the loops must say about it: start - first, or None where the check is the plant's own)
PLANTS = {}
for _adv in (19, 20, 40, 60, 61, 63, 64, 65, 79, 80, 81):   # a pure run of L bases advances `start` by L - 11 (strides 20 first, then whatever is left)
    PLANTS[f"advance_{_adv}"] = (run_end(30, 30 + _adv + 10), _adv)
PLANTS["hole_at_10_stride_20_jumps_it"] = (run_end(30, 85, holes=(40,)), 45)
PLANTS["hole_at_20_stride_15_goes_on"] = (run_end(30, 130, holes=(50,)), 90)      # 15 x 6 with the shared register exhausted on the way
PLANTS["reaches_window_minus_1"] = (run_end(100, 159), 49)
PLANTS["would_pass_window_170"] = (run_end(100, 170), 49)                          # forward: + 5, + 3
PLANTS["would_pass_window_172"] = (run_end(100, 172), 49)                          # forward: + 5, + 5
_e = run_end(100, 172)
_e[171] = "C"
PLANTS["forward_5_3_1"] = (_e, 49)                                                 # forward: + 5, + 3 (over the C), + 1
PLANTS["forward_stops_at_174"] = (run_end(100, 200), 49)                           # forward: + 5, + 5, + 1 to n - 1
PLANTS["entry_at_0"] = (run_end(0, 40), 30)
PLANTS["entry_at_149"] = (run_end(149, 190), 0)
PLANTS["n_inside_the_run"] = (run_end(30, 80, n_at=(50, 51, 66)), None)            # exact T excludes N
PLANTS["n_ends_the_run"] = (run_end(30, 120, n_at=tuple(range(60, 68))), None)


def both(T, G, first, window=WINDOW):
    a, b = {}, {}
    r_loop, r_mask = fm.tail_loops(T, G, first, window, a), fm.tail_masks(T, G, first, window, b)
    assert r_loop == r_mask, (hex(T), hex(G), first, r_loop, r_mask)
    return r_loop, a, b


@pytest.mark.parametrize("name", sorted(PLANTS))
def test_plants(sor, name):
    end, adv = PLANTS[name]
    codes = codes_of(end)
    T, G, first = fm.masks_of(codes)
    assert first >= 0
    (start, endpos, end1), loops, slow = both(T, G, first)
    got = sor.find_polyt(codes[:WINDOW + 25])       # the scan hands the finder the first window + polyATlength + 10 bases of an end
    assert got is not None and (int(got[0]), int(got[1])) == (first + 1, end1), (got, first, end1)
    if adv is not None:
        assert start - first == adv, (start, first)
    if name == "hole_at_10_stride_20_jumps_it":
        assert not (G >> (first + 10)) & 1 and (G >> (first + 20)) & 1 and loops["go"][0] >= 2
    if name == "hole_at_20_stride_15_goes_on":
        assert not (G >> (first + 20)) & 1 and (G >> (first + 15)) & 1 and loops["go"][:2] == [1, 7] and slow["ext"] >= 1
    if name.startswith("advance_8") or name == "advance_79":
        assert (slow["ext"] >= 1) == (adv >= 80)            # the stride-20 register holds four probes: 80 exhausts it
    if name == "reaches_window_minus_1":
        assert start == WINDOW - 1 and end1 == 160
    if name.startswith("would_pass") or name.startswith("forward_"):
        assert start == WINDOW - 1 and end1 == {"would_pass_window_170": 172, "would_pass_window_172": 174, "forward_5_3_1": 173, "forward_stops_at_174": 175}[name]
    if name == "entry_at_0":
        assert first == 0
    if name == "entry_at_149":
        assert first == 149 and end1 == 175
    if name == "n_inside_the_run":
        assert all(not (T >> p) & 1 for p in (50, 51, 66))
    if name == "n_ends_the_run":
        assert end1 == 60


def _bits(positions):
    m = 0
    for p in positions:
        m |= 1 << p
    return m


def test_structured_masks():
    """the cases bases cannot reach, and the registers' edges, as masks"""
    full = (1 << 175) - 1
    # the shared register of strides 15 .. 1: every probe of stride s set up to an advance of 63, 64, 65 (a register's width and one either side) and
    # of two registers.  Stride 15 is the one whose probes no larger stride shares: there the advance and the slow path are known in advance
    for s in (15, 10, 5, 4, 3, 2, 1):
        for reach in (44, 59, 60, 62, 63, 64, 65, 66, 127, 128, 129):
            first = 3
            G = _bits(first + k for k in range(s, reach + 1, s)) & ((1 << WINDOW) - 1)
            (start, _, _), loops, slow = both(full, G, first)
            if s == 15:
                assert start == first + s * (reach // s)
                assert (slow["ext"] >= 1) == (reach >= 60), (s, reach)       # the probes 15, 30, 45, 60 are all the register holds
    # the stride-20 register: advances of 60, 80, 100, 140 (a window's width plus or minus one probe)
    for k in (3, 4, 5, 7):
        G = _bits(20 * j for j in range(1, k + 1))
        (start, _, _), _, slow = both(full, G, 0)
        assert start == 20 * k and (slow["ext"] >= 1) == (k >= 4)
    # a hole at start + 10 with start + 20 set; a hole at start + 20 with start + 15 set
    assert both(full, _bits([30, 50]), 10)[0][0] == 50
    assert both(full, _bits([25, 40]), 10)[0][0] == 40
    # the walk back.  no back position at all: result 4
    for first in (0, 7, 60, 149):
        T = _bits(range(0, 175, 2))                     # no two adjacent T's
        (start, endpos, end1), _, _ = both(T, 0, first)
        assert start == first and endpos == 4
    # the highest back position just inside the window (its fifth position) and just outside (its fourth): endpos0 = first + 14, window from endpos0 - 40 on
    first = 100
    base = first + 14 - fm.BACK_BELOW
    for e, outside in ((base + 4, False), (base + 3, True), (base + 5, False), (base - 20, True)):
        T = _bits(range(e - 4, e + 1))
        (_, endpos, _), loops, slow = both(T, 0, first)
        assert endpos == e and loops["back"] == first + 14 - e and (slow["back"] == 1) == outside
    # positions 4 and 5: 4 is where the walk ends anyway, 5 is the lowest position that can pass
    for first in (0, 20, 26, 27, 60):
        assert both(_bits(range(0, 5)), 0, first)[0][1] == 4
        assert both(_bits(range(1, 6)), 0, first)[0][1] == 5
        assert both(_bits(range(0, 6)), 0, first)[0][1] == 5
    # forward steps that leave the window: a long run behind a short walk back
    for first in (0, 50, 120, 149):
        (_, endpos, end1), _, slow = both(full, 0, first)
        assert endpos == first + 14 and end1 == 175 and (slow["fwd"] >= 1) == (first + 14 + 23 < 174)
    # + 5, + 3 and + 1 that stop at n - 1 = 174
    for top, want in ((174, 175), (173, 174), (171, 172), (169, 170)):
        assert both(_bits(range(140, top + 1)), 0, 149)[0][2] == want


@pytest.mark.parametrize("seed", range(8))
def test_random_masks(seed):
    """40,000 pairs of masks per seed (320,000 in all): T and G drawn independently and at several densities, `first` anywhere below the window --
    the tails agree on any masks, not only on those a read can produce"""
    rng = random.Random(7000 + seed)
    wmask = (1 << WINDOW) - 1

    def draw(bits, dens):
        x = rng.getrandbits(bits)
        for _ in range(dens):
            x |= rng.getrandbits(bits)
        return x

    slow_seen = [0, 0, 0]
    for i in range(40_000):
        T = draw(192, i % 4)                    # 50 %, 75 %, 88 %, 94 % T
        if i % 7 == 0:                          # long gaps: the walk back leaves its window
            T &= ~(((1 << rng.randrange(20, 70)) - 1) << rng.randrange(0, 150))
        G = draw(WINDOW, (i // 4) % 5) & wmask
        if i % 5 == 0:                          # long runs of probes: the registers are exhausted
            G |= (((1 << rng.randrange(40, 150)) - 1) << rng.randrange(0, 100)) & wmask
        first = rng.randrange(0, WINDOW)
        _, _, slow = both(T, G, first)
        for j, k in enumerate(("ext", "back", "fwd")):
            slow_seen[j] += slow[k] > 0
    assert all(n > 100 for n in slow_seen), slow_seen   # the slow paths were part of it


def test_other_windows():
    """windows that end on and next to a word of the probe mask (tests/test_scan_lanes_gpu.py test_finder_window)"""
    rng = random.Random(7100)
    for window in (150, 149, 129, 128, 97, 1):
        for _ in range(3000):
            T = rng.getrandbits(192) | rng.getrandbits(192)
            G = (rng.getrandbits(window) | rng.getrandbits(window) | rng.getrandbits(window)) & ((1 << window) - 1)
            both(T, G, rng.randrange(0, window), window)


# ---- the end-of-read sums -----------------------------------------------------------------------------------------------------------------
def _loop_f32(k12, k10):
    """countIndelsMismatchesEndOfRead's sum as the reference adds it: k12 times (float)((double)e + 1.2), then k10 times e + 1.0f"""
    e = np.float32(0.0)
    for _ in range(k12):
        e = np.float32(np.float64(e) + np.float64(1.2))
    for _ in range(k10):
        e = np.float32(e + np.float32(1.0))
    return e


# ---- two more adapter ties (tests/test_scan_lazy_cpu.py pins the fold; its keys are 0, 1.0 and 1.2: one error column at most) ------------------
# the 10-mer with two substitutions: ne = 2, nmis = 2 (acceptable); the keys of a pair differ in k12 alone (2.4 against 1.2: two error columns over
# the last two read bases against one) and in k10 alone (2.0 against 1.0)
K12_HI, K12_LO = "CTTCCGATAA", "ATTCCGATAT"
K10_HI, K10_LO = "CTTCCAACCT", "ATTCCGCTCT"
MORE_TIES = [((K12_HI, K12_LO), 1), ((K12_LO, K12_HI), 0), ((K10_HI, K10_LO), 1), ((K10_LO, K10_HI), 0)]


def test_more_adapter_ties(sor):
    from test_scan_lazy_cpu import AD_POS, _a_pos, _nw_stats, ad_counts, tie_end
    from test_scan_queue_gpu import _c_end

    f32 = np.float32
    want = {K12_HI: _loop_f32(2, 0), K12_LO: _loop_f32(1, 0), K10_HI: _loop_f32(0, 2), K10_LO: _loop_f32(0, 1)}   # (k12, k10) of each key
    for s, key in want.items():
        st = _nw_stats(sor, AD[2], s)
        assert st["ne"] == 2.0 and st["nmis"] == 2 and f32(st["end5"]) == key, (s, st)
    for slices, win in MORE_TIES:
        end = tie_end(slices)
        assert ad_counts([end, _c_end()]) == [2, 0]                     # the two planted candidates and no other
        assert _a_pos(sor, end)[0] == AD_POS[win]                       # the smaller key wins, first or second
        assert all(_a_pos(sor, tie_end((s,)))[0] == AD_POS[0] for s in slices)   # each alone is found: the pair ties on ne
