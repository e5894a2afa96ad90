"""The chunks of tests/uparsecases.py really hold the edges they are named for, and tests/uparsemodel.py agrees with what the suite already
trusts (no GPU): tests/test_uparse_edges_gpu.py runs these chunks through K-UPARSE."""
import os
import re

import numpy as np
import pytest

import pymodel_group as pg
import uparsecases as uc
import uparsemodel as um

import __graft_entry__ as graft


def _expected(sor, cid):
    return um.expected(sor, cid, uc.case(cid))


def _blocks(names):
    return [sum(len(nm.encode()) for nm in names[a:a + 64]) for a in range(0, len(names), 64)]


def test_name_stage_is_the_kernels(pkg):
    src = open(os.path.join(graft.PKG_DIR, "csrc", "smi_umi_stage.hip")).read()
    m = re.findall(r"constexpr int kNameStage = (\d+);", src)
    assert len(m) == 1 and int(m[0]) == uc.NAME_STAGE
    assert "64 * (kNameStage + 4)" in src and "sizeof(stage) - 16" in src and uc.FLAT_LIMIT == 64 * (uc.NAME_STAGE + 4) - 16 == 20720


@pytest.mark.parametrize("five", [False, True])
def test_long_name_chunks_take_the_row_staging(pkg, five):
    a = uc.long_name_cases("a", five)[0]
    assert len(a) == 64 and _blocks(a)[0] > uc.FLAT_LIMIT
    lens = [len(nm) for nm in a]
    for n in (30, uc.NAME_STAGE, uc.NAME_STAGE + 1, uc.NAME_STAGE + 4):
        assert lens.count(n) >= 2, n
    assert sum(650 < n < 760 for n in lens) >= 10                                   # about 700 characters ...
    mark = [max(nm.find("_FWD_"), nm.find("_REV_")) for nm in a]
    assert sum(m > uc.NAME_STAGE and n > 650 for m, n in zip(mark, lens)) >= 10     # ... with the marker behind character 320
    # a needed tag value that starts behind character 320 while the marker lies in front of it
    behind = [nm for nm, m in zip(a, mark) if 0 <= m < 100 and all(nm.find(t, m) > uc.NAME_STAGE for t in ("_AE=", "_bc=", "_bcEnd=", "_X=", "_Q="))]
    assert len(behind) >= 10
    # X= values that straddle character 320, one of them inside the window's bases; markers that straddle it at every cut
    x0 = [nm.find("_X=", m) + 3 for nm, m in zip(a, mark) if m >= 0 and "_X=" in nm]
    assert {uc.NAME_STAGE - 17, uc.NAME_STAGE - 10, uc.NAME_STAGE - 30, uc.NAME_STAGE - 42} <= set(x0)
    lo, hi = (uc.POS - 1, uc.POS + 12) if five else (uc.X_LEN - uc.POS - 13, uc.X_LEN - uc.POS)      # indices of the window's bases inside X=
    assert any(s + lo < uc.NAME_STAGE <= s + hi for s in x0)
    assert {uc.NAME_STAGE - 4, uc.NAME_STAGE - 3, uc.NAME_STAGE - 1, uc.NAME_STAGE} <= set(mark)
    assert a[mark.index(uc.NAME_STAGE - 3)][uc.NAME_STAGE - 3:uc.NAME_STAGE + 2] == "_REV_"
    # b: a flat wave, one that is not, a partial flat one
    b = uc.long_name_cases("b", five)[0]
    blk = _blocks(b)
    assert len(b) == 135 and blk[0] <= uc.FLAT_LIMIT < blk[1] and blk[2] <= uc.FLAT_LIMIT
    # c: flat, with one name of 900 characters in front of 58 others
    c = uc.long_name_cases("c", five)[0]
    assert len(c) == 64 and _blocks(c)[0] <= uc.FLAT_LIMIT and len(c[5]) == 900 and max(len(nm) for nm in c[:5] + c[6:]) < 200
    for names, floor in ((a, 40), (b, 40), (c, 1)):
        assert um.long_names(names, uc.NAME_STAGE) >= floor


@pytest.mark.parametrize("five", [False, True])
def test_cigar_chunks_reach_every_return_of_the_walk(pkg, sor, five):
    from sicelore_amd import lib as libmod

    rows, groups = uc.cigar_layout(five)
    names, flags, pos0, cigars, kw = uc.finish(rows, five_prime=five)
    tags, n_done, recs = um.expect(sor, names, flags, pos0, cigars, **kw)
    assert n_done == len(names)
    branches, ops, labels = {}, set(), set()
    for g in groups:
        r = recs[g["probe"]]
        assert r["read_pos"] == g["rp"], g["label"]                                 # PS= / AE= moved the read position as meant
        br = um.ref_position_branch(g["cigar"], g["start"], g["rp"])
        walked = pg.ref_position_at_read_position(g["cigar"], g["start"], g["rp"])
        assert (walked is None) == (br in ("zero", "behind_far")), g["label"]
        assert libmod.ref_position_at_read_position_raw(cigars[g["probe"]], g["start"], g["rp"]) == walked
        assert r["position"] == (None if g["flag"] & 4 else walked)
        if not g["flag"] & 4:
            branches.setdefault(br, set()).add(g["label"])
        ops |= {op for op, _ in g["cigar"]}
        labels.add(g["label"])
        # the region tells the position to the base: one base off and the link of 499 between the probe and its anchors breaks
        mine = tags[g["probe"]]["region"]
        pos, rev = [x["position"] for x in recs], [x["reverse"] for x in recs]
        if g["expect"] == "with":
            assert mine >= 0 and mine == tags[g["anchors"][-1]]["region"], g["label"]
            pos[g["probe"]] += g["shift"]
        else:
            assert mine == -1 and tags[g["anchors"][-1]]["region"] >= 0, g["label"]
            pos[g["probe"]], rev[g["probe"]] = g["where"], False            # where a walk that misses the rule would put it
        if g["exact"]:
            assert pg.group_sams(pos, rev)[0] != [t["region"] for t in tags], g["label"]
    assert set(branches) == {"zero", "in_front", "inside", "behind_near", "behind_far"}
    assert {"negative", "lead_s_even", "lead_s_odd", "in_i_gap1", "in_i_gap7", "in_i_gap8"} <= branches["in_front"]
    assert {"block_first", "block_last", "behind_n", "behind_d", "eq_first", "x_inside", "h_ignored", "p_ignored"} <= branches["inside"]
    assert {"behind_299", "no_cigar_near"} <= branches["behind_near"] and {"behind_300", "no_cigar_far"} <= branches["behind_far"]
    assert ops == set("MIDNSHP=X") and {"unmapped", "reverse_alone", "reverse_with_anchors"} <= labels
    # the integer halving shows: gaps of 7 and 8 give the same offset, and the leading clip's rule differs by parity of the start
    by = {g["label"]: g for g in groups if g["shift"] < 0}
    p = lambda l: recs[by[l]["probe"]]["position"] - by[l]["start"]  # noqa: E731
    assert p("in_i_gap7") == 100 + 6 - 3 and p("in_i_gap8") == 100 + 7 - 4
    assert by["lead_s_even"]["start"] % 2 != by["lead_s_odd"]["start"] % 2


@pytest.mark.parametrize("five", [False, True])
@pytest.mark.parametrize("ul", [8, 10, 12])
def test_window_chunks_stand_on_both_sides_of_the_limits(pkg, sor, five, ul):
    names, flags, pos0, cigars, kw = uc.window_cases(five, ul)
    recs = um.records(names, flags, pos0, cigars, **kw)
    lim = uc.window_pos_limits(ul)
    by = {nm.split("_FWD_")[0]: i for i, nm in enumerate(names)}

    def pos_of(i):
        d = um.scan(names[i])
        return d["bc"]["end"] - d["ae"] + 3 if five else d["ae"] + 3 - d["bc"]["end"]
    want = {"w0": (0, False), "w1": (lim["first_legal"], True), "w2": (lim["last_legal"], True), "w3": (lim["first_illegal"], False)}
    for rid, (pos, has) in want.items():
        for c in "01":
            i = by[f"{rid}c{c}"]
            assert pos_of(i) == pos and (recs[i]["window"] is not None) == has and recs[i]["has_bc"], (rid, c)
    assert lim["last_legal"] + ul + 1 == uc.X_LEN == lim["first_illegal"] + ul
    d = um.scan(names[by["xec0"]])
    assert d["x"] == "" and recs[by["xec0"]]["window"] is None and recs[by["xec0"]]["has_bc"]
    for c in "01":
        w = recs[by[f"xn{c}"]]["window"]
        assert w[2] == 15 and w[5] == 15 and sum(v == 15 for v in w) == 2              # N and a lower-case letter: code 15
    assert recs[by["nqc0"]]["window"] is None and recs[by["nqc0"]]["has_bc"] and "_X=" in names[by["nqc0"]] and "_Q=" not in names[by["nqc0"]]
    assert not recs[by["ncc0"]]["has_bc"] and "_ed=" in names[by["ncc0"]] and "_bc=" not in names[by["ncc0"]]


@pytest.mark.parametrize("five", [False, True])
def test_q_chunks_make_a_misread_quality_visible(pkg, sor, five):
    """per form a set of two reads: with the members' Q texts exchanged the model's centre is the other read"""
    a, _, _ = _expected(sor, "q-5p" if five else "q-3p")
    names, flags, pos0, cigars, kw = uc.q_cases(five, exchanged=True)
    b, _, _ = um.expect(sor, names, flags, pos0, cigars, **kw)
    plain = uc.case("q-5p" if five else "q-3p")[0]
    for (i, j), (form, other) in zip(uc.q_group_rows(), uc.Q_FORMS):
        assert f"_Q={form}_" in plain[i] and f"_Q={other}_" in plain[j] and f"_Q={other}_" in names[i]
        hi, lo = (i, j) if np.float32(form) > np.float32(other) else (j, i)
        assert a[i]["center"] == a[j]["center"] == hi and b[i]["center"] == b[j]["center"] == lo, form
    assert [f for f, _ in uc.Q_FORMS] == ["12", "12.3", ".5", "7.", "007.25", "1234.567", "0"]


@pytest.mark.parametrize("five", [False, True])
def test_group_key_chunk_holds_its_sets(pkg, sor, five):
    rows, sets = uc.group_key_layout(five)
    names, flags, pos0, cigars, kw = uc.finish(rows, five_prime=five)
    tags, n_done, recs = um.expect(sor, names, flags, pos0, cigars, **kw)
    assert 110 <= len(names) <= 130 and n_done == len(names)
    bc = lambda label: {recs[i]["bc"] for i in sets[label]}  # noqa: E731
    diff = lambda a, b: [k for k in range(16) if a[k] != b[k]]  # noqa: E731
    (b0,), (b1,), (b2,), (b3,) = bc("base"), bc("first"), bc("last"), bc("mid")
    assert diff(b0, b1) == [0] and diff(b0, b2) == [15] and diff(b0, b3) == [7]
    assert bc("allA") == {"A" * 16} and bc("allT") == {"T" * 16}
    for label in ("base", "first", "last", "mid", "allA", "allT", "three"):
        assert len(sets[label]) == 3 and all(tags[i]["flags"] & um.CLUSTERED and tags[i]["center"] in sets[label] for i in sets[label]), label
    assert len(sets["one"]) == 1 and not tags[sets["one"][0]]["flags"] & um.CLUSTERED and tags[sets["one"][0]]["flags"] & um.HAS_U7
    assert len(sets["two"]) == 2 and all(tags[i]["flags"] & um.CLUSTERED for i in sets["two"])
    # two sets whose members alternate; inside each the centre is the first member in input order, which only a stable sort keeps first
    a, b = sets["ilA"], sets["ilB"]
    assert sorted(a + b) == list(range(min(a), min(a) + 6)) and a == sorted(a) and b == sorted(b) and a[0] < b[0] < a[1] < b[1] < a[2] < b[2]
    for s in (a, b):
        assert all(tags[i]["center"] == s[0] for i in s)
        ws = np.array([recs[i]["window"] for i in reversed(s)], dtype=np.uint8)           # the same set in another order: another centre
        asg, _ = sor.umi_cluster_group(sor.umi_matrix(ws).reshape(-1), 3, np.array([recs[i]["q"] for i in reversed(s)], dtype=np.float32))
        assert list(reversed(s))[int(asg["center"][0])] != s[0]
    # the same barcode (and UMI) in two regions
    ra, rb = {tags[i]["region"] for i in sets["sameA"]}, {tags[i]["region"] for i in sets["sameB"]}
    assert len(ra) == len(rb) == 1 and ra != rb and min(ra | rb) >= 0 and bc("sameA") == bc("sameB")
    assert all(tags[i]["center"] in sets["sameA"] for i in sets["sameA"]) and all(tags[i]["center"] in sets["sameB"] for i in sets["sameB"])
    assert {int(pos0[i]) for i in sets["sameB"]} == {int(pos0[i]) + 5000 for i in sets["sameA"]}


def test_tail_chunks_end_on_a_read_that_counts(pkg, sor):
    assert uc.TAIL_CUTS == [1, 2, 63, 64, 65, 128, 129, 255, 256, 257] and len(uc.tail_records()) == 300
    for five in (False, True):
        full = uc.finish(uc.tail_records(five), five_prime=five)
        recs = um.records(*full[:4], **full[4])
        for n in uc.TAIL_CUTS:
            assert recs[n - 1]["position"] is not None and recs[n - 1]["window"] is not None, n
        assert any(r["position"] is None for r in recs) and any(r["window"] is None for r in recs)
    names, flags, pos0, cigars, kw = uc.tail_cases(129, keep_data_end=True)
    tags, n_done, _ = um.expect(sor, names, flags, pos0, cigars, **kw)
    assert 129 // 3 <= n_done < 129 and all(t["region"] == -1 and t["flags"] == 0 for t in tags[n_done:])
    assert any(t["flags"] for t in tags[:n_done])


def test_marker_tag_and_number_chunks_hold_their_names(pkg, sor):
    for five in (False, True):
        names = uc.marker_cases(five)[0]
        recs = um.records(*uc.marker_cases(five)[:4], five_prime=five)
        assert sum("_FWD_" in nm and nm.find("_FWD_") < nm.find("_REV_") for nm in names) >= 2
        assert sum(nm.count("_REV_") == 2 for nm in names) >= 2 and sum(nm.startswith("_FWD_") for nm in names) >= 2
        none = [i for i, nm in enumerate(names) if "_FWD_" not in nm and "_REV_" not in nm]
        assert len(none) >= 6 and all(not recs[i]["has_bc"] and recs[i]["position"] is None for i in none)
        for i, nm in enumerate(names):          # whatever stands in front of the marker or a second time behind it is not what was read
            if nm[:2] in ("fr", "rr", "pr", "du"):
                assert recs[i]["bc"] not in (None, "T" * 16, "G" * 16) and recs[i]["window"] is not None, nm
        names = uc.tag_order_cases(five)[0]
        last = {re.search(r"_([A-Za-z]+)=[^_]*$", nm).group(1) for nm in names if re.search(r"_([A-Za-z]+)=[^_]*$", nm)}
        assert last == set(uc.SEVEN)
        assert any(0 <= nm.find("_bcEnd=") < nm.find("_bc=") for nm in names) and any(0 <= nm.find("_ed_sec=") < nm.find("_ed=") for nm in names)
        assert any("_bcStart=" not in nm and "_bc=" in nm for nm in names) and any("_T=" in nm and "_rk=" in nm and "_PE=" in nm for nm in names)
        for limit in (0, 1, -1):
            names, flags, pos0, cigars, kw = uc.number_cases(five, limit)
            assert kw["bc_edit_limit"] == limit
            recs = um.records(names, flags, pos0, cigars, **kw)
            by = {nm.split("_FWD_")[0]: i for i, nm in enumerate(names)}
            for n, v in enumerate(uc.EDGE_INTS):
                assert f"_PS={v}_" in names[by[f"ps{n}"]] and f"_bcEnd={v}_" in names[by[f"be{n}"]]
                assert recs[by[f"be{n}"]]["has_bc"] and recs[by[f"be{n}"]]["window"] is None
            assert uc.EDGE_INTS == ["0", "-0", "-5", "2147483647", "-2147483648"]
            assert sorted(len(um.scan(names[by[f"ae{n}c0"]])["ae"].__str__()) for n in range(3)) == [1, 5, 10]
            assert all(recs[by[f"ae{n}c0"]]["window"] is not None for n in range(3))
            assert (recs[by["psx"]]["position"] is not None) == five and recs[by["psx"]]["has_bc"]
            assert not recs[by["edx"]]["has_bc"] and recs[by["bex"]]["has_bc"] and recs[by["bex"]]["window"] is None
            for n, ed in enumerate((0, 1, 2)):
                assert f"_ed={ed}_" in names[by[f"ed{n}c0"]] and recs[by[f"ed{n}c0"]]["has_bc"] == (limit < 0 or ed <= limit), (limit, ed)


def test_every_device_case_holds_only_names_the_kernel_evaluates(pkg):
    n = 0
    for cid in uc.CASES:
        for nm in uc.case(cid)[0]:
            assert uc.evaluated_on_device(nm), (cid, nm)
            assert " " not in nm and "\t" not in nm
            n += 1
    assert n > 2500
    kinds = {k: kind for k, _, kind in uc.FALLBACKS}
    assert set(kinds) == {"bc15", "bc17", "bcN", "ps_plus", "ps_blank", "q_exp", "q_neg", "q_4dec", "q_8dig", "q_29", "ae_zeros", "ae_11", "bcend_11",
                          "ae_absent", "ae_12x", "ends_in_rev"}
    assert {k for k, v in kinds.items() if v == "error"} == {"ae_11", "ae_absent", "ae_12x", "ends_in_rev"}
    plain = uc.finish(uc.ordinary(191, 70))[0]
    for which in kinds:
        names = uc.fallback_cases(which)[0]
        assert len(names) == 70 and [i for i in range(70) if names[i] != plain[i]] == [uc.FALLBACK_AT]
        assert [i for i, nm in enumerate(names) if not uc.evaluated_on_device(nm)] == [uc.FALLBACK_AT], which
    q29 = re.search(r"_Q=([^_]*)", uc.fallback_cases("q_29")[0][uc.FALLBACK_AT]).group(1)
    assert len(q29) == 29


@pytest.mark.parametrize("cid", list(uc.CASES))
def test_model_agrees_with_the_host_units_and_meets_its_floors(pkg, sor, cid):
    """positions and regions of every chunk through the product's host functions (smi_ref_position_at_read_position, smi_region_group), which
    tests/test_group.py holds to the oracle and to the reference's bytecode; and the least every chunk must exercise on the device"""
    from sicelore_amd import lib as libmod

    names, flags, pos0, cigars, kw = uc.case(cid)
    tags, n_done, recs = _expected(sor, cid)
    for i, r in enumerate(recs):
        got = None
        if r["read_pos"] is not None and not int(flags[i]) & 4:
            got = libmod.ref_position_at_read_position_raw(cigars[i], int(pos0[i]) + 1, r["read_pos"])
        assert got == r["position"], (cid, names[i])
    region, done = libmod.region_group([r["position"] for r in recs], [r["reverse"] for r in recs], max_dist=500,
                                       keep_data_end=bool(kw.get("keep_data_end")))
    assert done == n_done and [x if i < done else -1 for i, x in enumerate(region)] == [t["region"] for t in tags]
    assert len(names) <= 300
    have = um.floors(tags, recs, names, uc.NAME_STAGE)
    need = um.least(cid)
    assert all(have[k] >= v for k, v in need.items()), (cid, have, need)


@pytest.mark.parametrize("five", [False, True])
def test_model_reads_odd_names_as_the_reference_does(pkg, five):
    """FastqRecordExt.getScanDatFromReadName executed from the reference's class files on names with one odd field
    (tests/golden/ref_exec_umi_odd_names.json): what it parsed is what the model parses; where it throws on AE= (or finds none) the model
    raises; where it throws on PS= / ed= / bcEnd= the model has no such field -- the product's reading, which this vector records as not the
    reference's"""
    import json

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_exec_umi_odd_names.json")) as f:
        data = json.load(f)
    assert "jvm_exec" in data["how"] and data["bytecode_steps"] > 0
    sec = [s for s in data["sections"] if s["five_prime"] == five][0]
    assert sec["reference_class"].startswith("com/rw/") and len(sec["cases"]) == 40
    n = dict(parsed=0, error=0, absent=0)
    for c in sec["cases"]:
        nm = c["name"]
        if "throws" not in c:
            d = um.scan(nm)
            assert (d["ae"], d["ps"], d["bc"]["ed"], d["bc"]["end"]) == (c["adapter_end"], c["polya_start"], c["bc_ed"], c["bc_end"]), nm
            assert np.float32(d["q"]) == np.float32(c["mean_qv"]), nm
            n["parsed"] += 1
        elif "AdapterInfoNotFound" in c["throws"] or "_AE=743_" not in nm:
            with pytest.raises(pkg.SmiError, match="AE="):
                um.scan(nm)
            assert not uc.evaluated_on_device(nm)
            n["error"] += 1
        elif "_Q=abc" not in nm:
            assert c["throws"] == "java/lang/NumberFormatException"
            d = um.scan(nm)
            gone = [k for k, v in (("PS", d["ps"]), ("ed", d["bc"]), ("bcEnd", d["bc"] and d["bc"]["end"])) if v is None]
            assert len(gone) >= 1 and all(f"_{k}=" in nm for k in gone), nm
            n["absent"] += 1
    assert n["parsed"] >= 20 and n["error"] >= 8 and n["absent"] >= 8, n
