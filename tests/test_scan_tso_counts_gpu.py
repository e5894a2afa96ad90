"""K-SCAN's TSO round on counts (csrc/smi_nw.h nw_counts: no tags, no walk) and phase C's second alignment of the few winners whose runs a rescue rule
reads -- the shipped kernels (which do both) and the generic ones (which walk every candidate) against the oracle, whole records, passes 2 (the 10-mer)
and 1 (the 22-mer).

Every plant is a pair of read ends on the all-C background (no 4-mer of the TSO occurs in it, so every gated position is planted).  What a plant IS is
proved on the CPU first, by the oracle's alignment statistics folded as the scan folds them (_winner): the winner's position, ne, nmis, ins, del and its
runs.  Then the plant under test is put at lane 0 (read 0's head), at lane 63 (read 31's tail) and on the last read's tail, in batches of 1, 33, 65 and
129 reads whose other reads carry a whole TSO on one end: those pass outright, so the planted ends are the only ones of their waves that can ask for the
second alignment -- in the batch of 65 the one on the last read's tail is alone in its wave, and in the batch of 1 alone altogether.

Every plant of the issue can be said in bases; none is left out."""
import ctypes
import math

import numpy as np
import pytest

from test_scan_lanes_gpu import TSO, _batch, _codes, _run_all, gm
from test_scan_lazy_cpu import TSO_CONSEC, TSO_NEITHER, TSO_TWO, tso_end, whole
from test_scan_queue_gpu import _c_end

pytestmark = pytest.mark.gpu

INSERTED = TSO[:8] + "TT" + TSO[8:]        # two bases too many in the middle: up moves there, and the pattern's last two bases fall off the 16-base slice
C = None                                   # an end that carries nothing

# name -> (head, tail, (head found, tail found)) of the read under test; None = all C
PLANTS = {
    "clean": (TSO, C, (True, False)),
    "needy_by_consec": (TSO_CONSEC, C, (True, False)),
    "needy_by_two": (TSO_TWO, C, (True, False)),
    "needy_by_neither": (TSO_NEITHER, C, (False, False)),
    # the same needy ends beside a partner that is found: no rescue rule is asked, whatever their runs are
    "needy_two_partner_found": (TSO_TWO, TSO, (False, True)),
    "needy_neither_partner_found": (TSO_NEITHER, TSO, (False, True)),
    "both_needy_consec_two": (TSO_CONSEC, TSO_TWO, (True, False)),       # consec rescues the head, so the second rule is not asked for the tail
    "both_needy_neither_consec": (TSO_NEITHER, TSO_CONSEC, (False, True)),
    "both_needy_two_two": (TSO_TWO, TSO_TWO, (True, True)),
    "both_needy_neither": (TSO_NEITHER, TSO_NEITHER, (False, False)),
    "trailing_read_gaps": (INSERTED, C, (True, False)),
}
NAMES = sorted(PLANTS)
NEEDY = (TSO_CONSEC, TSO_TWO, TSO_NEITHER)


def _end(sl):
    return _c_end() if sl is None else tso_end(sl)


def _winner(sor, end):
    """the TSO fold of one end (AdapterTSOanalyzer L96-106: first best accepted position, the jump behind a candidate with ne > 5) over the oracle's
    statistics of every gated slice -> dict of the winner, or None"""
    L = sor.lib()
    L.sor_nw_stats.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    o9, f2 = np.zeros(9, dtype=np.int32), np.zeros(2, dtype=np.float32)
    text = "".join(end)
    tm = gm.gate_masks(_codes([(end, _c_end())])[:1], TSO, gm.TSO_WINDOW)[0]
    best, skip, win = math.inf, 0, None
    for p in (np.nonzero(tm)[0] + 1).tolist():
        if p < skip:
            continue
        sl = text[p - 1:p + 15]
        assert L.sor_nw_stats(TSO.encode(), sl.encode(), o9.ctypes.data, f2.ctypes.data, None) == 0
        ne = float(f2[0])
        if math.floor(np.float32(ne) + np.float32(0.5)) <= 5 and ne < best:
            best = ne
            win = dict(pos=p, ne=ne, nmis=int(o9[2]), ins=int(o9[5]), dele=int(o9[4]), consec=int(o9[6]), two=int(o9[7]), strings=sor.nw_strings(TSO, sl))
        if ne > 5.0:
            skip = p + max(1, math.floor(np.float32(ne - 5.0) + np.float32(0.5)) - 1)
    return win


@pytest.fixture(scope="module")
def winners(sor):
    return {sl: _winner(sor, _end(sl)) for sl in (TSO, INSERTED) + NEEDY}


def test_what_the_plants_are(winners):
    w = winners[TSO]
    assert (w["nmis"], w["ins"], w["dele"], w["ne"]) == (0, 0, 0, 0.0)
    for sl in NEEDY:                                        # present (accepted by round(ne) <= 5) and not passed (nmis > 5)
        w = winners[sl]
        assert round(w["ne"]) <= 5 and w["nmis"] > 5, sl
    lead = [len(winners[sl]["strings"][0]) - len(winners[sl]["strings"][0].lstrip("-")) for sl in NEEDY]
    assert max(lead) > 0                                    # leading template gaps are how ne stays small beside many mismatches
    assert winners[TSO_CONSEC]["consec"] >= 8
    assert winners[TSO_TWO]["consec"] < 8 and winners[TSO_TWO]["two"] >= 12
    assert winners[TSO_NEITHER]["consec"] < 8 and winners[TSO_NEITHER]["two"] < 12
    w = winners[INSERTED]                                   # read gaps that end the alignment are not deletions: del != ins
    assert w["strings"][2].endswith("--") and (w["ins"], w["dele"]) == (2, 0) and w["nmis"] <= 5


def _plant_batch(n, name):
    """n reads: the plant on read 0 (lane 0 = its head), mirrored on read 31 (lane 63 = its tail) and on the last read -> [(head, tail)], {read: mirrored}"""
    head, tail, _ = PLANTS[name]
    ends, where = [], {}
    for i in range(n):
        if i == 0:
            ends.append((_end(head), _end(tail)))
            where[i] = False
        elif i == 31 or i == n - 1:
            ends.append((_end(tail), _end(head)))
            where[i] = True
        else:
            ends.append((whole(i), _c_end()) if i % 2 else (_c_end(), whole(i)))
    return ends, where


def _tso(exp):
    return np.stack([exp["tso_start"], exp["tso_end"]], 1)


@pytest.mark.parametrize("n", [1, 33, 65, 129])
def test_plants_in_batches(pkg, sor, gpu_ctx, monkeypatch, winners, n):
    for k, name in enumerate(NAMES):
        ends, where = _plant_batch(n, name)
        ra, qa, offs = _batch(ends, np.random.default_rng(9500 + 37 * n + k))
        exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)        # shipped == generic == oracle, passes 2 and 1
        t = _tso(exp)
        found = PLANTS[name][2]
        for rd, mirrored in where.items():
            assert (t[rd] != 0).tolist() == list(found[::-1] if mirrored else found), (name, n, rd)
        rest = [i for i in range(n) if i not in where]
        assert ((t[rest] != 0).sum(1) == 1).all()                            # the other reads: their whole TSO and nothing else
        if name == "trailing_read_gaps":                                    # the end of the match = position + 15 + ins - del, with del = 0
            w = winners[INSERTED]
            assert t[0, 0] == w["pos"] + 15 + w["ins"] - w["dele"] == w["pos"] + 17


def test_a_needy_end_in_every_wave(pkg, sor, gpu_ctx, monkeypatch):
    """129 reads = five waves, each with one end that asks for the second alignment, on lanes 3, 10, 17, 24 and on the last read's head; every other
    end of the batch carries nothing at all, so the waves run no other TSO alignment"""
    lanes = {w: (7 * w + 3) % 64 for w in range(4)}
    lanes[4] = 0
    ends = [[_c_end(), _c_end()] for _ in range(129)]
    for w, lane in lanes.items():
        ends[32 * w + lane // 2][lane & 1] = tso_end((TSO_TWO, TSO_CONSEC, TSO_NEITHER)[w % 3])
    ra, qa, offs = _batch([tuple(e) for e in ends], np.random.default_rng(9601))
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
    t = _tso(exp) != 0
    assert t.sum() == 4                                                     # waves 0, 1, 3, 4 are rescued, wave 2's end (two runs of five) is not
    for w, lane in lanes.items():
        assert t[32 * w + lane // 2, lane & 1] == (w % 3 != 2)


def test_needy_ends_on_every_lane(pkg, sor, gpu_ctx, monkeypatch):
    """a wave whose 64 ends all ask: both ends of every read are needy, in every combination of the three slices"""
    sl = (TSO_CONSEC, TSO_TWO, TSO_NEITHER)
    ends = [(tso_end(sl[i % 3]), tso_end(sl[(i // 3) % 3])) for i in range(32)]
    ra, qa, offs = _batch(ends, np.random.default_rng(9701))
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
    t = _tso(exp) != 0
    assert t[0].tolist() == [True, True] and t[8].tolist() == [False, False] and t[1].tolist() == [False, True]   # consec | consec, neither | neither, two | consec
