"""The alignment statistics K-SCAN computes only where a rule reads them (consec / best_two of the TSO winner inside the rescue rules, end5 on a tie of
two acceptable adapter candidates, endn == 0 in the pass-1 filter): the cases that reach those rules, found once by a seeded search with the oracle
(sor_nw_stats / scan_read_3p over mutated TSOs and adapters planted on the all-C background), frozen here as literals, and proved by the oracle for what
each one is.  tests/test_scan_lazy_gpu.py plants them into waves; the waves' candidate counts are proved here by the CPU model of the gate."""
import ctypes

import numpy as np
import pytest

from test_scan_gpu import AD
from test_scan_lanes_gpu import E, TSO, _batch, _codes, _put, _rc, gm
from test_scan_queue_gpu import PE, _c_end, _offsets, _pairs, _tso_masks

P = 10                                    # where the TSO slices are planted (scan position)
# TSO slices whose winner is accepted (round(ne) <= 5) with nmis > 5: present, not passed
TSO_CONSEC = "TCGAGTACATTG"               # rescued by consec >= 8
TSO_TWO = "AAACGCAGTACATACG"              # consec 7: rescued by best_two >= 12 only
TSO_NEITHER = "AACGGAGAGAGTAACATGC"       # exactly two runs of 5 (best_two 10, consec 5): rescued by neither
TSO_FIRST_RUN = "AACAGGTACATGG"           # the winner (position 7) ends in a run of 8 matches, which starts the walk and does not count
# with maxNeedlemanMismatches 7 and minTSO_NeedlemanConsecutiveMatches 4 both ends are rescued and their nmis differ by more than 3
RULE_HEAD, RULE_TAIL, RULE_KNOBS = "TGTTTTAACGCCATGG", "TACGAAGTACAC", dict(tso_scan_max_mm=7, tso_scan_min_consec=4, tso_scan_min_two_best=32)   # (32: the largest the knob takes; two stretches of a 16-mer never reach it)
# the 10-mer with one substitution: ne = 1, nmis = 1 (acceptable), end5 = 0 / 1.0 / 1.2 by where the substitution lies
LO, HI10, HI10B, HI12 = "ATTCCGATCT", "CTTCCAATCT", "CTTCCCATCT", "CTTCCGATAT"
BAD4, OK4 = "CTTCCAAAGA", "AAAACGATCT"    # both gated, ne = 4, nmis 4 > maxMM; the second ends in six matches and is acceptable by them, the first is not
AD_POS = (20, 55, 90)
# (planted slices, index of the winner): the fold's rule is key < incumbent's key, first of its group
TIES = [((LO, HI10), 0), ((HI10, LO), 1), ((HI12, HI10, LO), 2), ((HI10, HI12, LO), 2), ((HI12, HI10, HI10B), 1), ((BAD4, OK4), 1), ((HI10, HI10B), 0),
        ((LO, HI12), 0), ((HI12, LO), 1)]
# pass 1: the winner's only error lies outside / inside the last minAdapter3pMatches = 8 read bases
PASS1_22 = ("ATACACGACGCTCTTCCGATCT", "CTACACGACGCTCTACCGATCT")
PASS1_10 = ("ATTCCGATCT", "CTACCGATCT")
MID = "ACG" * 13 + "A"


# ---- builders ----------------------------------------------------------------------------------------------------------------------------
def tso_end(sl, p=P):
    e = _c_end()
    if sl:
        _put(e, p, sl)
    return e


def tie_end(slices, pe=PE, polyt=True):
    """an all-C end with the slices at AD_POS, in front of a T run that ends at pe"""
    e = _c_end()
    if polyt:
        _put(e, pe - 40, "T" * 41)
    for p, s in zip(AD_POS, slices):
        _put(e, p, s)
    return e


def read_of(head, tail):
    return "".join(head) + MID + _rc("".join(tail))


def _nw_stats(sor, pattern, sl):
    L = sor.lib()
    L.sor_nw_stats.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    o9, f2, row = np.zeros(9, dtype=np.int32), np.zeros(2, dtype=np.float32), np.zeros(64, dtype=np.int32)
    assert L.sor_nw_stats(pattern.encode(), sl.encode(), o9.ctypes.data, f2.ctypes.data, row.ctypes.data) == 0
    return dict(term6=int(o9[1]), nmis=int(o9[2]), consec=int(o9[6]), two=int(o9[7]), ne=float(f2[0]), end5=float(f2[1]))


def _tso_rec(sor, head, tail, mm=5, consec=8, two=12):
    """(tso_start, tso_end) of one read under the given TSO limits"""
    par = sor.set_tso_params(sor.default_scan_params(), TSO, 90, mm, consec, two)
    rc, r = sor.scan_read_3p(read_of(head, tail), None, AD[2], params=par)
    assert rc == 0
    return int(r["tso_start"]), int(r["tso_end"])


def _a_pos(sor, head, adapter=AD[2], qual=None):
    """(scan position of the accepted adapter or 0, the record)"""
    rd = read_of(head, _c_end())
    rc, r = sor.scan_read_3p(rd, qual, adapter)
    assert rc == 0
    return (len(rd) - int(r["adapter_start"]) + 1 if r["adapter_found"] else 0), r


# ---- the waves of the GPU tests ----------------------------------------------------------------------------------------------------------
def whole(i):
    return tso_end(TSO, 3 + i % 30)   # a whole TSO: nmis 0, passes outright


def rescue_wave(lane, with_lane=True, sl=TSO_TWO):
    """every end carries a whole TSO but `lane` (a slice that needs the rescue) and its partner (nothing, so that the rescue decides the read's record)"""
    ends = [whole(i) for i in range(64)]
    ends[lane ^ 1] = _c_end()
    ends[lane] = tso_end(sl) if with_lane else _c_end()
    return ends


BOTH = {5: (TSO_CONSEC, TSO_TWO), 9: (TSO_TWO, TSO_TWO), 12: (TSO_NEITHER, TSO_CONSEC), 20: (TSO_NEITHER, TSO_NEITHER), 27: (TSO_CONSEC, TSO_CONSEC),
        30: (TSO_FIRST_RUN, None)}


def both_wave():
    """reads whose two ends both need the rescue (read: head, tail), among reads that pass outright"""
    ends = [whole(i) for i in range(64)]
    for rd, (h, t) in BOTH.items():
        ends[2 * rd], ends[2 * rd + 1] = tso_end(h), tso_end(t)
    return ends


def rule_wave():
    ends = [whole(i) for i in range(64)]
    ends[6], ends[7] = tso_end(RULE_HEAD), tso_end(RULE_TAIL)
    ends[40], ends[41] = tso_end(RULE_TAIL), tso_end(RULE_HEAD)
    return ends


def ties_wave():
    """one round: 20 owners on alternating sides, each with one arrangement of TIES; -> ends, [(read, side, arrangement)]"""
    ends, plan = [], []
    for i in range(32):
        own = tie_end(TIES[i % len(TIES)][0]) if i < 20 else _c_end()
        ends += [own, _c_end()] if i % 2 == 0 else [_c_end(), own]
        if i < 20:
            plan.append((i, i % 2, i % len(TIES)))
    return ends, plan


def seam_wave():
    """65 adapter candidates: two on each of 31 owners, three on the last (numbers 62, 63 | 64): its incumbent is settled in round 1 (HI12, then HI10 by
    the tie) and the candidate that ties with it and wins (LO) is aligned in round 2"""
    ends = []
    for i in range(32):
        own = tie_end(TIES[i % 2][0]) if i < 31 else tie_end((HI12, HI10, LO))
        ends += [own, _c_end()] if i % 2 == 0 else [_c_end(), own]
    return ends


def ties_5p():
    """the arrangements without a polyT, for the 5' scan with no polyA asked for (both ends gated over positions 1 .. 110)"""
    ends = []
    for i in range(32):
        own = tie_end(TIES[i % len(TIES)][0], polyt=False) if i < 31 else tie_end((HI12, HI10, LO), polyt=False)
        ends += [own, _c_end()] if i % 2 == 0 else [_c_end(), own]
    return ends


def pass1_reads():
    """reads 0, 1: the 22-mer pair; reads 2, 3: the 10-mer pair (complete adapter in front of it, so that pass 1 finds it too)"""
    ends = []
    for s in PASS1_22:
        e = _c_end()
        _put(e, PE - 40, "T" * 41)
        _put(e, 30, s)
        ends += [e, _c_end()]
    for s in PASS1_10:
        e = _c_end()
        _put(e, PE - 40, "T" * 41)
        _put(e, 30, AD[1][:12] + s)
        ends += [_c_end(), e]
    return ends


def pass1_batch():
    return _batch(_pairs(pass1_reads()), np.random.default_rng(7301))


def partial_wave(n):
    """n reads, the rescue on the last read's tail (the last active lane)"""
    ends = []
    for i in range(n - 1):
        ends += [whole(i), _c_end()]
    return ends + [_c_end(), tso_end(TSO_TWO)]


def ad_counts(ends, n_pos=PE - 12):
    """adapter candidates per end: the 10-mer's gate over positions 1 .. n_pos of the ends that carry a planted slice"""
    codes = _codes(_pairs(ends))
    return [int(gm.gate_masks(codes[i:i + 1], AD[2], n_pos)[0].sum()) if "".join(e) != "C" * E else 0 for i, e in enumerate(ends)]


# ---- what each frozen case is ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sl,by_consec,by_two", [(TSO_CONSEC, True, False), (TSO_TWO, False, True), (TSO_NEITHER, False, False)])
def test_tso_slices_need_the_rescue(sor, sl, by_consec, by_two):
    head, c = tso_end(sl), _c_end()
    assert _tso_rec(sor, head, c, consec=99, two=99) == (0, 0)          # not passed by nmis: nothing without the rescue rules ...
    assert _tso_rec(sor, head, c, consec=1, two=1)[0] != 0              # ... yet present: accepted with round(ne) <= 5
    assert (_tso_rec(sor, head, c, consec=8, two=99)[0] != 0) == by_consec
    assert (_tso_rec(sor, head, c, consec=99, two=12)[0] != 0) == by_two
    assert (_tso_rec(sor, head, c)[0] != 0) == (by_consec or by_two)     # the shipped limits
    # raising the limit that rescues it to 99 changes the record
    if by_consec:
        assert _tso_rec(sor, head, c, consec=99, two=99) != _tso_rec(sor, head, c, consec=8, two=99)
    if by_two:
        assert _tso_rec(sor, head, c, consec=8, two=99) != _tso_rec(sor, head, c, consec=8, two=12)


def test_tso_consec_slice_has_one_stretch(sor):
    """TSO_CONSEC is rescued by the first rule: its second rule alone would not rescue it at 12 (one stretch of 8)"""
    head, c = tso_end(TSO_CONSEC), _c_end()
    assert _tso_rec(sor, head, c, consec=99, two=8)[0] != 0 and _tso_rec(sor, head, c, consec=99, two=9) == (0, 0)


def test_longest_run_starts_the_walk(sor):
    head, c = "".join(tso_end(TSO_FIRST_RUN)), _c_end()
    sl = head[7 - 1:7 - 1 + 16]
    st, dots = _nw_stats(sor, TSO, sl), sor.nw_strings(TSO, sl)[1]
    assert len(dots) - len(dots.rstrip(".")) == 8 and st["consec"] == 3            # a run of 8 at the start of the walk, and it does not count
    assert round(st["ne"]) <= 5 and st["nmis"] > 5
    assert _tso_rec(sor, list(head), c) == (0, 0)                                  # 8 would rescue it, 3 does not ...
    assert _tso_rec(sor, list(head), c, consec=3, two=99)[0] != 0 and _tso_rec(sor, list(head), c, consec=4, two=99) == (0, 0)   # ... and 3 is what the rule reads


def test_two_runs_of_five(sor):
    head, c = tso_end(TSO_NEITHER), _c_end()
    st = _nw_stats(sor, TSO, "".join(head)[13 - 1:13 - 1 + 16])
    assert (st["consec"], st["two"]) == (5, 10) and st["nmis"] == 6 and round(st["ne"]) == 5
    assert _tso_rec(sor, head, c, consec=99, two=10)[0] != 0 and _tso_rec(sor, head, c, consec=99, two=11) == (0, 0)


def test_nmis_rule_fires_after_a_rescue(sor):
    kw = dict(mm=7, consec=4, two=32)
    h, t, c = tso_end(RULE_HEAD), tso_end(RULE_TAIL), _c_end()
    assert _tso_rec(sor, h, c, mm=7, consec=99, two=99) == (0, 0) and _tso_rec(sor, c, t, mm=7, consec=99, two=99) == (0, 0)   # neither passes by nmis
    assert _tso_rec(sor, h, c, **kw)[0] != 0 and _tso_rec(sor, c, t, **kw)[1] != 0       # each alone is rescued ...
    got = _tso_rec(sor, h, t, **kw)
    assert got[0] == 0 and got[1] != 0                                                   # ... together the one with more mismatches is dropped
    got = _tso_rec(sor, t, h, **kw)
    assert got[0] != 0 and got[1] == 0


def test_adapter_slices(sor):
    for s, key in ((LO, 0.0), (HI10, 1.0), (HI10B, 1.0), (HI12, 1.2)):
        st = _nw_stats(sor, AD[2], s)
        assert st["ne"] == 1.0 and st["nmis"] == 1 and abs(st["end5"] - key) < 1e-6
    bad, ok = _nw_stats(sor, AD[2], BAD4), _nw_stats(sor, AD[2], OK4)
    assert bad["ne"] == ok["ne"] == 4.0 and bad["nmis"] == ok["nmis"] == 4 and not bad["term6"] and ok["term6"]
    assert _a_pos(sor, tie_end((BAD4,)))[0] == 0 and _a_pos(sor, tie_end((OK4,)))[0] == AD_POS[0]


@pytest.mark.parametrize("k", range(len(TIES)))
def test_adapter_tie_winner(sor, k):
    slices, win = TIES[k]
    pos, r = _a_pos(sor, tie_end(slices))
    assert pos == AD_POS[win]
    # every slice alone is found where it is planted (but BAD4, which is not acceptable): the end's best ne is shared by all of them
    for j, s in enumerate(slices):
        e = _c_end()
        _put(e, PE - 40, "T" * 41)
        _put(e, AD_POS[j], s)
        assert _a_pos(sor, e)[0] == (0 if s == BAD4 else AD_POS[j])


def test_pass1_pair(sor):
    ra, qa, offs = pass1_batch()
    _, e1 = sor.scan_batch_3p(ra, qa, offs, AD[1])
    _, e2 = sor.scan_batch_3p(ra, qa, offs, AD[2])
    assert e1["adapter_found"][:2].tolist() == [1, 1] and e1["pass1_ok"][:2].tolist() == [1, 0]     # the 22-mer: endn == 0 or not
    assert e2["adapter_found"][2:].tolist() == [1, 1] and e2["pass1_ok"][2:].tolist() == [1, 0]     # the 10-mer with qualities
    assert e1["adapter_nmis"][:2].tolist() == [1, 1] and e2["adapter_nmis"][2:].tolist() == [1, 1]  # the pair differs in where the error lies only


# ---- the waves' candidate counts, by the CPU model of the gate ---------------------------------------------------------------------------
@pytest.mark.parametrize("lane", [0, 63])
def test_planted_rescue_wave(lane):
    tm = _tso_masks(rescue_wave(lane))
    assert tm[lane].any() and not tm[lane ^ 1].any() and (tm.sum(1) > 0).sum() == 63
    tm = _tso_masks(rescue_wave(lane, with_lane=False))
    assert not tm[lane].any() and (tm.sum(1) > 0).sum() == 62


def test_planted_both_wave():
    tm = _tso_masks(both_wave())
    assert (tm.sum(1) > 0).sum() == 63            # (read 30's tail carries nothing)


def test_planted_ties_wave():
    ends, plan = ties_wave()
    cnt = ad_counts(ends)
    assert sum(cnt) <= 64 and len(plan) == 20     # one round
    for rd, side, k in plan:
        assert cnt[2 * rd + side] >= len(TIES[k][0])
    assert not _tso_masks(ends).any()             # and no TSO candidate at all


def test_planted_seam_wave():
    cnt = ad_counts(seam_wave())
    own = [c for c in cnt if c]
    assert own == [2] * 31 + [3]
    off = _offsets(own)
    assert off[31] == 62 and off[32] == 65        # the last owner holds 62, 63 | 64


def test_planted_ties_5p():
    cnt = ad_counts(ties_5p(), 110)
    assert sum(cnt) > 64 and all(c >= 2 for c in cnt if c)


@pytest.mark.parametrize("n", [1, 33, 65])
def test_planted_partial(n):
    tm = _tso_masks(partial_wave(n))
    assert tm[-1].any() and not tm[-2].any()
