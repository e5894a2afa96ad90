"""The hand-built K-CHIM cases (tests/chimcases.py) mean what they say: every intent is asserted with pymodel_chimera's own functions, every exactly-at / one-past
pair separates its threshold, and oracle and model agree on every read of every batch.  No GPU."""
import pytest

import chimcases as cc
import pymodel_chimera as pm
from pymodel_scan import NeedlemanMatch, enc, kmers_matching, needleman

CASES = cc.all_cases()
BY_NAME = cc.by_name()
NAMES = [c["name"] for c in CASES]
_MODEL = {}


def model(read, fp):
    key = (read, fp)
    if key not in _MODEL:
        splits, multi, ms = cc.model(read, fp)
        _MODEL[key] = (splits, multi, ms)
    return _MODEL[key]


def tso_scan(read, fp, reverse):
    """-> (accepted scan positions, the gated positions the walk visits [(pos, nErrors, delta)])"""
    cfg = cc.CFG[fp]
    pat4 = pm.rc4(enc(cfg["tso"])) if reverse else enc(cfg["tso"])
    s4 = enc(read)
    acc = pm.pos_below_max(pm.scan_kmers_internal(s4, 70, len(s4) - 70, pat4, cfg["tso_max"], 2), cfg["tso_max"]) or []
    return sorted(p for p, _ in acc), cc.walk(s4, pat4, cfg["tso_max"])


def n_gated(read, fp, reverse):
    cfg = cc.CFG[fp]
    pat4 = pm.rc4(enc(cfg["tso"])) if reverse else enc(cfg["tso"])
    s4 = enc(read)
    return sum(1 for p in range(70, min(len(s4) - len(pat4), len(s4) - 70) + 1) if kmers_matching(s4, pat4, p) >= 2)


def ad_window(s4, at, cfg):
    if at["nuc"] == pm.T:
        start = at["begin"] - cfg["bc_umi"] - 40
        return s4[start - 1:start + 50]
    end = at["end"] + cfg["bc_umi"] + 40
    return pm.rc4(s4[end - 51:end])


def outcome(sor, case, name=None):
    """what a twin must differ in: the oracle's result of the target, or the model quantity the family names"""
    read, fp = case["reads"][case["target"]], case["five_prime"]
    d = case["intent"].get("differs") if name is None else name
    if d == "stretches":
        return len(pm.at_scan(enc(read)))
    if d == "accepted":
        return len(tso_scan(read, fp, False)[0])
    if d == "gated":
        return n_gated(read, fp, False)
    if d == "kept_offsets":  # the best-score offsets of the one adapter window that survive the "< 2 apart" removal
        cfg, s4 = cc.CFG[fp], enc(read)
        sub, ad4 = ad_window(s4, pm.at_scan(s4)[0], cfg), enc(cfg["ad"])
        rslt = pm.scan_kmers_internal(sub, 1, len(sub) - len(ad4), ad4, cfg["ad_max"], 3)
        offs = list(rslt[min(rslt)])
        return len([o for i, o in enumerate(offs) if i == 0 or abs(o - offs[i - 1]) >= 2])
    return cc.expected(sor, read, fp)


def test_plane_formula_is_the_library_s(pkg):
    from sicelore_amd import lib as libmod

    for total, n in ((0, 1), (31, 1), (32, 1), (17000, 1), (700_000, 400), (123_457, 63)):
        assert cc.planes_words(total, n) == libmod.read_planes_words(total, n)
    assert cc.plane_word([0, 64, 100], 2, 33) == (100 >> 5) + 10 + 1


@pytest.mark.parametrize("name", NAMES)
def test_case_means_what_it_says(sor, name):
    case = BY_NAME[name]
    fp, reads, t, it = case["five_prime"], case["reads"], case["target"], case["intent"]
    cfg = cc.CFG[fp]
    read = reads[t]
    s4 = enc(read) if "N" not in read or len(read) <= cc.MODEL_MAX else None
    rc_, splits, multi, n_matches = cc.expected(sor, read, fp)
    assert rc_ == 0
    if len(read) <= cc.MODEL_MAX:
        m_splits, m_multi, m_ms = model(read, fp)
        assert (splits, multi, n_matches) == (m_splits, m_multi, len(m_ms)), name
    if "phase" in it:
        q, word, bit = it["phase"]
        assert cc.plane_word(cc.offsets_of(reads), t, q) % cc.TILE == word and q % 32 == bit
        if name.split("_")[1] == "S1":
            kind = name.split("_")[2]
            if kind == "ftso":
                assert tso_scan(read, fp, False)[0] == [q + 1]
            elif kind == "rtso":
                assert tso_scan(read, fp, True)[0] == [q + 1]
            else:
                ats = pm.at_scan(s4)
                assert [(a["nuc"], a["begin"]) for a in ats] == [(pm.T if kind == "polyT" else pm.A, q + 1)]
                tile = lambda x: cc.plane_word(cc.offsets_of(reads), t, x) // cc.TILE  # noqa: E731
                if (word, bit) == (255, 31):
                    assert tile(q + 14) == tile(q) + 1                          # the 15-base window straddles the seam
                if kind == "polyA" and word == 255:
                    assert tile(q + 14 + cfg["bc_umi"] + 40) == tile(q) + 1     # the adapter's search range runs into the next tile
                if kind == "polyT" and word == 0:
                    assert tile(q - cfg["bc_umi"] - 40) == tile(q) - 1          # ... or lies in the tile before
        if "front" in it:
            assert reads[t - 1] == it["front"] and tso_scan(read, fp, False)[0] == [70]
    if "n_matches" in it:
        assert n_matches == it["n_matches"]
    if "n_splits" in it:
        assert len(splits) == it["n_splits"]
    if "multi" in it:
        assert multi == it["multi"]
    if "long_sites" in it:
        assert len(read) == 17000 and n_matches == it["long_sites"]
        w = [cc.plane_word(cc.offsets_of(reads), t, q) // cc.TILE for q in (500, 8500, 16400 + len(cfg["ad"]) + cfg["bc_umi"])]
        assert w[0] < w[1] < w[2]  # three tiles
        if name.endswith("S3_last"):
            total, n = cc.offsets_of(reads)[-1], len(reads)
            assert (cc.planes_words(total, n) // 4) % cc.TILE != 0  # the final tile is partly beyond the stride
    if "tso_at" in it:
        reverse, pos, found = it["tso_at"]
        assert (pos in tso_scan(read, fp, reverse)[0]) == found
        assert read[pos - 1:pos - 1 + len(cfg["tso"])] == (cc.rc(cfg["tso"]) if reverse else cfg["tso"])
        assert pos in (69, 70, len(read) - 70, len(read) - 69)
    if "trigger" in it:
        nuc, pos, found = it["trigger"]
        ats = pm.at_scan(s4)
        assert [(a["nuc"], a["begin"]) for a in ats] == ([(pm.T if nuc == "T" else pm.A, pos + 1)] if found else [])
        assert read[pos] == read[pos + 1] == nuc and pos in (cc.OFF - 1, cc.OFF - 2, len(read) - cc.OFF - 1, len(read) - cc.OFF)
    if "doubled" in it:
        nuc, found = it["doubled"]
        assert read[cc.OFF:cc.OFF + 14].count(nuc) == 10 and (read[cc.OFF + 13] == nuc) == bool(found)  # threshold - 1 = 10 of 15 * 0.70 -> 11
        assert [a["begin"] for a in pm.at_scan(s4)] == ([cc.OFF] if found else [])
    if "begins_apart" in it:
        _, _, ms = model(read, fp)
        rev = [m for m in ms if m["rev"]]
        fwd = [m for m in ms if not m["rev"]]
        assert len(rev) == 1 and len(fwd) == 1 and fwd[0]["begin"] - rev[0]["begin"] == it["begins_apart"]
    if "ad_begins_apart" in it:
        nuc, d = it["ad_begins_apart"]
        ats = pm.at_scan(s4)
        for at in ats:
            pm.adapter_scan(s4, at, enc(cfg["ad"]), cfg["ad_max"], cfg["bc_umi"])
        starts = [at["matches"][0] for at in ats if at["matches"] and at["nuc"] == (pm.T if nuc == "T" else pm.A)]
        assert len(starts) == 2 and starts[1] - starts[0] == d  # both adapters align; the rule alone decides how many enter
    if "sorted_apart" in it:
        p0, d, third = it["sorted_apart"]
        pat4 = enc(cfg["tso"])
        lst = pm.pos_below_max(pm.scan_kmers_internal(s4, 70, len(s4) - 70, pat4, cfg["tso_max"], 2), cfg["tso_max"])
        assert [p for p, _ in lst] == [p0 + d, p0, third] and lst[0][1] < lst[1][1] <= lst[2][1]  # the sort puts the later position first
        assert third - p0 == 121
    if "best_offsets" in it:
        d = it["best_offsets"]
        ats = pm.at_scan(s4)
        assert len(ats) == 1
        sub, ad4 = ad_window(s4, ats[0], cfg), enc(cfg["ad"])
        rslt = pm.scan_kmers_internal(sub, 1, len(sub) - len(ad4), ad4, cfg["ad_max"], 3)
        offs = list(rslt[min(rslt)])
        assert len(offs) == 2 and offs[1] - offs[0] == d   # two offsets share the best score
        kept = [o for i, o in enumerate(offs) if i == 0 or abs(o - offs[i - 1]) >= 2]
        assert kept == (offs[:1] if d == 1 else offs)      # 1 apart: the second is removed; 2 apart: both stay
        assert all(NeedlemanMatch(needleman(ad4, sub[o - 1:o - 1 + len(ad4)])).nmis <= cfg["ad_max"] for o in offs)
        _, _, ms = model(read, fp)
        assert [m["begin"] for m in ms] == [ats[0]["begin"] - cfg["bc_umi"] - 40 + offs[0] - 1]  # the match starts at the first offset
    if "ad_nmis" in it:
        want, accepted = it["ad_nmis"]
        ats = pm.at_scan(s4)
        assert len(ats) == 1
        sub, ad4 = ad_window(s4, ats[0], cfg), enc(cfg["ad"])
        full = pm.scan_kmers_internal(sub, 1, len(sub) - len(ad4), ad4, 99, 3)  # every gated position of the window with its score
        o = min((k, v[0]) for k, v in full.items())[1]
        assert NeedlemanMatch(needleman(ad4, sub[o - 1:o - 1 + len(ad4)])).nmis == want
        assert (n_matches == 1) == accepted
    if "decoy_at" in it:
        g, d = it["decoy_at"]
        acc, visited = tso_scan(read, fp, False)
        v = {p: (ne, dl) for p, ne, dl in visited}
        assert g in v and v[g][0] > cfg["tso_max"] and g + d in acc  # gated, visited, over the bound; the site d behind it is accepted
        assert not any(g < p < g + d for p in acc)
    if "closure" in it:
        # between the reads of K1 only the decoy's membership in the closure differs: around the two sites nothing else passes the gate
        g, d = it["decoy_at"]
        L = len(cfg["tso"])
        for reverse in (False, True):
            pat4 = pm.rc4(enc(cfg["tso"])) if reverse else enc(cfg["tso"])
            lo = g + 30 - L if reverse else g - 32   # (the reverse pattern's closure is its own: only what overlaps the bases that differ counts)
            near = [p for p in range(lo, g + d + L + 1) if kmers_matching(s4, pat4, p) >= 2]
            assert near == ([] if reverse else [g, g + d]), (reverse, near)
    if "chain" in it:
        chain, site = it["chain"]
        acc, visited = tso_scan(read, fp, False)
        v = {p: ne for p, ne, _ in visited}
        assert all(p in v and v[p] > cfg["tso_max"] for p in chain) and acc == [site]
        gaps = [b - a for a, b in zip(chain + [site], (chain + [site])[1:])]
        assert sorted(set(gaps)) == ([31] if name.endswith("chain_31") else [31, 32]) and chain[-1] - chain[0] + gaps[-1] >= 300
    if it["family"] == "K":
        # chimcases.walk is a copy of scan_kmers_internal's loop that also returns what it visits: what it accepts is what the model accepts
        acc, visited = tso_scan(read, fp, False)
        assert sorted(p for p, ne, _ in visited if not pm.jround(ne) > cfg["tso_max"]) == acc
    if "skip" in it:
        g, site, found = it["skip"]
        acc, visited = tso_scan(read, fp, False)
        v = {p: (ne, dl) for p, ne, dl in visited}
        assert g in v and v[g][0] > cfg["tso_max"]
        assert g + v[g][1] == (site if found else site + 1)           # the skip lands on the site / one position past it
        assert (site in v) == found and (site in acc) == found         # ... which the reference then visits and accepts / never visits
        pat4 = enc(cfg["tso"])
        assert kmers_matching(s4, pat4, site) >= 2 and not pm.jround(cc.count_errors(needleman(pat4, s4[site - 1:site - 1 + len(pat4)]))) > cfg["tso_max"]
    if "stretches" in it:
        assert len(pm.at_scan(s4)) == it["stretches"]
    if "accepted" in it and "queue" not in it:
        reverse, k = it["accepted"]
        assert len(tso_scan(read, fp, reverse)[0]) == k
    if "gated" in it:
        reverse, k = it["gated"]
        if "N" in read:
            assert set(read) == {"N"} and n_gated(read, fp, reverse) == k > 2048  # the model: every scanned position passes the gate
            o = cc.offsets_of(reads)
            assert cc.plane_word(o, t, 69) // cc.TILE == cc.plane_word(o, t, len(read) - 71) // cc.TILE  # ... and they lie in one tile
        else:
            assert n_gated(read, fp, reverse) == k and n_gated(read, fp, not reverse) <= 512
    if "queue" in it:
        counter, what, cap, per_read = it["queue"]
        n = len(reads)
        assert per_read * n < cap  # the queue has its minimum size
        total = n_st = 0
        for r in sorted(set(reads)):
            r4 = enc(r)
            if what == "stretches":
                k = len(pm.at_scan(r4))
            elif what == "ad_entries":
                ad4 = enc(cfg["ad"])
                k = 0
                for at in pm.at_scan(r4):
                    sub = ad_window(r4, at, cfg)
                    gated = [p for p in range(1, len(sub) - len(ad4) + 1) if kmers_matching(sub, ad4, p) >= 3]
                    k += len(gated)
                n_st += len(pm.at_scan(r4)) * reads.count(r)
            else:
                k = len(tso_scan(r, fp, False)[0])  # accepted positions are under the bound: each one is queued
            total += k * reads.count(r)
        assert total > cap and n_st <= 4096, (total, cap, n_st)  # (the adapter queue is reached only if the stretches fit theirs)


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["intent"].get("twin")])
def test_twin_differs(sor, name):
    case = BY_NAME[name]
    twin = BY_NAME[name[:3] + case["intent"]["twin"]]
    assert outcome(sor, case) != outcome(sor, twin, case["intent"].get("differs"))
    a, b = case["reads"][case["target"]], twin["reads"][twin["target"]]
    assert abs(len(a) - len(b)) <= 100


@pytest.mark.parametrize("five_prime", [False, True])
def test_oracle_and_model_agree_on_every_read(sor, five_prime):
    seen = set()
    for case in CASES:
        if case["five_prime"] != five_prime:
            continue
        for read in case["reads"]:
            if read in seen:
                continue
            seen.add(read)
            rc_, splits, multi, n_matches = cc.expected(sor, read, five_prime)
            assert rc_ == 0, case["name"]  # no case declares a read the reference would throw on
            if len(read) <= cc.MODEL_MAX:
                m_splits, m_multi, m_ms = model(read, five_prime)
                assert (splits, multi, n_matches) == (m_splits, m_multi, len(m_ms)), case["name"]
    assert len(seen) > 90
