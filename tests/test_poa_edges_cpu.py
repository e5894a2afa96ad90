"""The cases of tests/poacases.py prove themselves without a GPU: the model (tests/consensusmodel.py, E as a prefix maximum opened from H')
gives what the literal reference gives (E cell by cell, opened from H, its own traceback); every traceback re-scored under rule 1 is worth
the best H; E1 >= g and E2 >= q in every alignment; each family does what it claims (the gap of exactly L between aligned flanks, the tie
of the two gap types at L = 2, the type-2 gap from L = 3 on, the group of 20, the three chains); and every mutant of the literal changes
the output of a named case, so a kernel with that mistake fails tests/test_poa_edges_gpu.py."""
import pytest

import consensusmodel as cm
import poacases as pc

# what the literal can afford cell by cell: everything but the 6,000-base molecule, and the two run families on a 200-base source (the 400-base
# ones go through the model only)
LITERAL = [("seam_lengths", ()), ("ins_runs", (200,)), ("del_runs", (200,)), ("low_complexity", ()), ("wide_groups", ()), ("many_reads", ())]
LITERAL_CASES = [pytest.param(fam, args, cid, id=cid) for fam, args in LITERAL for cid in pc.family(fam, *args)]
EVERY = [(fam, ()) for fam in pc.FAMILIES] + [("ins_runs", (200,)), ("del_runs", (200,))]


def trace(reads):
    return pc.model_trace(reads, "int32" if max(map(len, reads)) > 3000 else "int64")


@pytest.mark.parametrize("fam,args,cid", LITERAL_CASES)
def test_literal_reference_equals_the_model(fam, args, cid):
    reads = pc.family(fam, *args)[cid]
    assert pc.literal_poa(reads) == pc.model(reads)


@pytest.mark.parametrize("fam,args", EVERY, ids=[f + "".join(map(str, a)) for f, a in EVERY])
def test_tracebacks_are_worth_the_best_h_and_e_stays_above_the_gap_open(fam, args):
    """rule 1 on the alignment the traceback returned == the end cell's H; E1 >= g and E2 >= q (H' >= 0 is part of every prefix maximum),
    which is why the int16 rows need no lower clamp"""
    n_dp = 0
    for cid, reads in pc.family(fam, *args).items():
        for k, r in enumerate(trace(reads)[1]):
            assert r["score"] == r["best"], f"{cid}, read {k}"
            if r["e1_min"] is not None:
                assert r["e1_min"] >= pc.G and r["e2_min"] >= pc.Q, f"{cid}, read {k}"
                assert r["best"] <= 5 * len(reads[k])
                n_dp += 1
    assert n_dp >= 2


def test_path_score_rejects_what_is_not_a_path():
    g = cm.Graph()
    cm.add_read(g, b"ACGTAC", [-1] * 6)
    assert pc.path_score(g, b"ACG", [0, 1, 2]) == 15
    assert pc.path_score(g, b"AGT", [0, 2, 3]) == 5 + 5 + 5 + pc.G                  # one node skipped
    assert pc.path_score(g, b"ATTC", [0, -1, -1, 1]) == 10 + pc.G + pc.E == 10 + pc.Q + pc.C   # L = 2: the two types tie
    assert pc.path_score(g, b"ATTTC", [0, -1, -1, -1, 1]) == 10 + pc.Q + 2 * pc.C
    assert pc.path_score(g, b"ATTTC", [0, -1, -1, -1, 1], one_gap_type=True) == 10 + pc.G + 2 * pc.E
    assert pc.path_score(g, b"AC", [1, 0]) is None and pc.path_score(g, b"AA", [0, 0]) is None
    assert pc.path_score(g, b"AC", [-1, -1]) == 0


def test_the_run_families_hold_the_listed_lengths_and_positions():
    small = (1, 2, 3, 4, 63, 64, 65)
    ins = {f"ins400-L{L}-p{p}" for L in small for p in pc.RUN_P} | {f"ins400-L130-p{p}" for p in (127, 128, 129)}
    assert set(pc.family("ins_runs")) == ins and len(ins) == 59
    dels = {f"del400-L{L}-p{p}" for L in small for p in pc.RUN_P} | {f"del400-L130-p{p}" for p in (127, 128, 129)}
    dels |= {f"del400-L130-p{p}-unbridged" for p in (62, 63, 64, 65)} | {f"del400-L{L}-p128-bubble" for L in pc.RUN_L}
    assert {c for c in pc.family("del_runs") if c.startswith("del")} == dels and len(dels) == 71
    assert len(pc.family("ins_runs", 200)) >= 50 and len(pc.family("del_runs", 200)) >= 50


def test_seam_lengths_are_exact():
    cases = pc.family("seam_lengths")
    assert [tuple(map(len, m)) for m in cases.values()] == [(n, n, n - 1, n + 1) for n in pc.SEAM_N]


def _parse(cid):
    f = cid.split("-")
    return int(f[1][1:]), int(f[2][1:])


@pytest.mark.parametrize("n_src", [400, 200])
def test_insertions_are_one_run_of_exactly_l_between_aligned_flanks(n_src):
    for cid, reads in pc.family("ins_runs", n_src).items():
        L, p = _parse(cid)
        r = trace(reads)[1][1]
        (pos, length), = r["ins"]
        assert length == L and abs(pos - p) <= 1 and not r["dels"], cid
        assert (r["left"], r["right"]) == (pos, n_src - pos), cid              # every base of both flanks is aligned
        if L == 2:
            assert r["score_one_type"] == r["score"] and pc.G + pc.E == pc.Q + pc.C, cid
        if L >= 3:
            assert r["score_one_type"] < r["score"], cid                        # the score needs the type-2 gap
        for k in (2, 3):                                                        # the clean copies go straight through
            assert trace(reads)[1][k]["best"] == 5 * n_src and not trace(reads)[1][k]["ins"] and not trace(reads)[1][k]["dels"]
        assert pc.model(reads)[0] == reads[0], cid                              # and outvote the insertion


@pytest.mark.parametrize("n_src", [400, 200])
def test_deletions_skip_exactly_l_nodes_between_aligned_flanks(n_src):
    n_open = 0
    for cid, reads in pc.family("del_runs", n_src).items():
        if not cid.startswith("del"):
            continue
        L, p = _parse(cid)
        k = 2 if cid.endswith("bubble") else 1
        r = trace(reads)[1][k]
        if cid.endswith("unbridged"):                                          # the 62..65-base flank earns less than the 526 the gap costs
            assert [x for x in r["dels"] if x[1] == L] == [] and r["best"] > 5 * len(reads[k]) + pc.gap_score(L), cid
            n_open += 1
            continue
        (pos, length), = r["dels"]
        assert length == L and abs(pos - p) <= 1 and not r["ins"], cid
        assert (r["left"], r["right"]) == (pos, n_src - L - pos), cid
        assert r["best"] == 5 * (n_src - L) + pc.gap_score(L), cid
        if L == 2:
            assert r["score_one_type"] == r["score"], cid
        if L >= 3:
            assert r["score_one_type"] < r["score"], cid
        if k == 2:
            # F walked through the bubble; for L <= 2 the node behind the stretch is also where the bubble closes: three edges come in
            assert trace(reads)[2]["max_indeg"] == (3 if L <= 2 else 2), cid
        assert pc.model(reads)[0] == reads[0], cid
    assert n_open == (4 if n_src == 400 else 0)


def test_wide_groups_reach_a_group_and_an_in_degree_of_20():
    cases = pc.family("wide_groups")
    for cid in ("wide-20", "wide-20-crossed"):
        st = trace(cases[cid])[2]
        assert (st["max_group"], st["max_indeg"]) == (20, 20), cid
    assert set(b"".join(cases["all-bytes"])) == set(range(256))
    cons, _counts = pc.model(cases["all-bytes"])
    assert {0x00, 0x0a, 0xff} <= set(cons)


def test_low_complexity_claims():
    cases = pc.family("low_complexity")
    recs = trace(cases["disjoint-ACG"])[1]
    assert [r["best"] for r in recs] == [0, 0, 0] and trace(cases["disjoint-ACG"])[2]["nodes"] == 300     # nothing aligns: three chains
    assert pc.model(cases["disjoint-ACG"]) == (b"A" * 100, [1] * 100)                                    # every bundle ties: the first
    recs = trace(cases["homopolymer-A"])[1]
    assert [r["best"] for r in recs[1:]] == [350, 650, 320]                # every cell on 70 diagonals holds the maximum: the first wins


def test_int16_extreme_reaches_exactly_30000():
    reads = pc.family("int16_extreme")["int16-6000"]
    recs = trace(reads)[1]
    assert (len(reads[0]), recs[1]["best"], recs[1]["nodes"]) == (6000, 30000, 6000)
    assert recs[2]["best"] == 500 and recs[3]["best"] > 0


# the mistake -> the cases of its target family that notice it (each is asserted: all of them have to)
MUTANTS = [
    ("chunk_carry", False, "ins_runs", (200,), ("ins200-L1-p64", "ins200-L2-p127", "ins200-L63-p64", "ins200-L65-p128", "ins200-L4-p192")),
    ("one_gap_type", True, "ins_runs", (200,), ("ins200-L63-p64", "ins200-L64-p127")),
    ("one_gap_type", True, "del_runs", (200,), ("del200-L63-p64", "del200-L65-p64-bubble", "del200-L3-p192")),
    ("f2_first", True, "del_runs", (200,), ("gap-ties-26", "gap-ties-41", "gap-ties-50")),
    ("last_max", True, "low_complexity", (), ("homopolymer-A", "dinucleotide-AC")),
    ("high_rank", True, "del_runs", (200,), ("del200-L1-p64-bubble", "del200-L2-p64-bubble")),
    ("no_ring", True, "wide_groups", (), ("wide-20-crossed",)),
]


@pytest.mark.parametrize("switch,value,fam,args,cids", MUTANTS, ids=[f"{m[0]}-{m[2]}" for m in MUTANTS])
def test_every_mutant_is_killed_by_named_cases(switch, value, fam, args, cids):
    """f2_first is not noticed by the clean-copy runs (F1 and F2 of equal value lie on the same chain there, so either order walks the same
    nodes); the gap-ties molecules, part of del_runs, are what kills it"""
    cases = pc.family(fam, *args)
    for cid in cids:
        assert pc.literal_poa(cases[cid], **{switch: value}) != pc.model(cases[cid]), f"{switch} survives {cid}"
