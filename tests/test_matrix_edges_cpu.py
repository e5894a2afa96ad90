"""The builders of tests/edgecases.py without a GPU: every case goes through the Python model, and the test asserts that the edge the case
is built for is really in it -- a generator that stops reaching its edge fails here, nothing is skipped or filtered out.  The expectations
known by construction (counts per cell, bases, qualities, assigned transcripts) are compared with the model, which so gets a second opinion
before any kernel is compared with it."""
import bammodel
import edgecases as ec
import isoformmodel as im
import snpmodel as sm


def _matrix_counts(text):
    return [int(v) for line in text.decode().split("\n")[1:-1] for v in line.split("\t")[3:]]


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------
def test_render_case_counts_by_construction_equal_the_model():
    c = ec.render_case()
    assert c["n_tail"] > 1000 and c["n_first"] == sum(c["counts"].values())       # repeats exist, all of them behind every first record
    seen = set()
    for n in (1, 63, 64, 65, 128, 129, 200):
        out, cnt, _pl = ec.snp_model("render", csv=ec.render_csv(n))
        mat, met, labels = ec.render_expected(n)
        assert out["snpmatrix.txt"] == mat and out["snpmetrics.txt"] == met and cnt["cells"] == n and cnt["rows"] == len(labels)
        assert cnt["kept"] < cnt["hits"] or n == 200                              # hit cells that are not listed
        assert cnt["kept"] > cnt["total_count"]                                   # distinct UMIs, not records
        head = mat.split(b"\n")[0].split(b"\t")
        assert n == 1 or (head[-1] == b"ZZ" and all(line.endswith(b"\t0") for line in mat.split(b"\n")[1:-1]))
        seen.update(_matrix_counts(mat))
    assert seen >= set(ec.COUNTS)
    for n, zz in ((201, True), (64, False), (65, False), (200, False)):            # C199 listed: all five rows; no ZZ: counts in the last column
        out, cnt, _pl = ec.snp_model("render", csv=ec.render_csv(n, zz))
        mat, met, labels = ec.render_expected(n, zz)
        assert out["snpmatrix.txt"] == mat and out["snpmetrics.txt"] == met and cnt["cells"] == n
        assert len(labels) == (ec.RENDER_ROWS if n >= 200 else 4)
        assert zz or sum(not line.endswith(b"\t0") for line in mat.split(b"\n")[1:-1]) >= (1 if n == 200 else 2)
    assert b"\t1001\n" in ec.render_expected(64, False)[0] and b"\t11\n" in ec.render_expected(200, False)[0]
    row0 = ec.render_expected(200)[0].split(b"\n")[1].split(b"\t")[3:]
    assert [int(v) for v in row0[58:69]] == list(ec.COUNTS) and len({len(v) for v in row0[60:68]}) == 4   # mixed widths over cells 63 | 64


def test_wide_case_reaches_six_digits():
    c = ec.wide_case()
    out, cnt, _pl = ec.snp_model("wide")
    mat, met, _labels = ec.wide_expected()
    assert out["snpmatrix.txt"] == mat and out["snpmetrics.txt"] == met
    vals = _matrix_counts(mat)
    assert max(vals) >= 100000 and {len(str(v)) for v in vals} == {1, 2, 3, 4, 5, 6}
    assert c["n_tail"] > 1000 and cnt["kept"] == c["n_first"] + c["n_tail"] > cnt["total_count"] == sum(ec.WIDE_COUNTS.values())


def test_render_blocks_break_around_the_widest_row():
    mat, _met, labels = ec.render_expected(201)
    rb = [ec.render_row_bytes(201, lab, 1001) for lab in labels]
    assert len(labels) == 5 and rb[0] > rb[1] == rb[2] == rb[3] == rb[4]
    assert b"\t1001" in mat.split(b"\n")[2]                                       # row 1 holds the widest count
    for name, (budget, blocks) in ec.render_budgets().items():
        assert ec.render_blocks(labels, 201, 1001, budget) == blocks, name
    layouts = [b for _n, b in ec.render_budgets().values()]
    assert [[0], [1, 2], [3, 4]] in layouts and [[0, 1], [2, 3], [4]] in layouts    # a break only in front of row 1, one only behind it
    assert layouts.count([[0], [1], [2], [3], [4]]) == 2                            # both around it; a budget smaller than any row


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------
def _candidates(bam, snp):
    """per record the lines K-SNP has to look at: same reference, same strand, [first, last] overlapping the alignment"""
    _t, refs, recs = bammodel.parse_bam(bam)
    lines = sm.parse_snp(snp, [nm for nm, _ln in refs])
    out = {}
    for r in recs:
        s = r["pos0"] + 1
        e = s + sm.reference_length(r["cigar"]) - 1
        out[r["name"]] = [L for L in lines if L["ref"] == r["ref_id"] and L["neg"] == bool(r["flag"] & 16) and L["arr"][0] <= e and L["arr"][-1] >= s]
    return out, lines, recs


def test_search_case_reaches_its_batches():
    c = ec.search_case()
    out, cnt, per_line = ec.snp_model("search")
    assert [(p["line"], p["hits"]) for p in per_line] == c["hits"] and all(p["lowRN"] == p["lowQV"] == 0 for p in per_line)
    labels = [ln.split("\t")[0] + "\t" + ln.split("\t")[1] + "\tna" for ln in out["snpmatrix.txt"].decode().split("\n")[1:-1]]
    assert labels == c["rows"]
    cand, lines, recs = _candidates(c["bam"], c["snp"])
    assert [len(cand[f"ov{n}"]) for n in ec.OVERLAPS] == list(ec.OVERLAPS) and max(len(v) for v in cand.values()) >= 129
    assert len(cand["short_only"]) == 401 and len(cand["spliced"]) == 401          # both also under `wide`
    # the wide line is the only candidate of wide_only, and only the running maximum finds it: every line sorted behind it ends in
    # front of that record
    assert [L["gene"] for L in cand["wide_only"]] == ["wide"]
    start = next(r["pos0"] + 1 for r in recs if r["name"] == "wide_only")
    chr1 = sorted((L for L in lines if L["ref"] == 0), key=lambda L: L["arr"][0])
    at = [L["gene"] for L in chr1].index("wide")
    behind = [L for L in chr1[at + 1:] if L["arr"][0] <= start + 99]
    assert len(behind) == 400 and all(L["arr"][-1] < start for L in behind)
    assert sum(L["arr"][0] == 3000010 for L in lines) == 5                        # several lines of one first position
    assert not cand["on_chr2"] and not cand["unmapped"] and any(L["chrom"] == "chr3" for L in lines)
    # inclusive borders
    by = {p["line"].split(",")[3]: p["hits"] for p in per_line}
    assert (by["b_before"], by["b_start"], by["b_end"], by["b_behind"]) == (0, 1, 1, 0)


def test_search_case_bad_attribute_on_the_record_only_the_wide_line_reaches():
    c = ec.search_case(bad_rn=True)
    try:
        sm.snp_matrix(c["bam"], c["snp"], c["csv"])
    except sm.SnpError as e:
        assert "read wide_only: attribute RN" in str(e)
    else:
        raise AssertionError("the model did not look at wide_only")


def test_table_case_every_listed_cell_once():
    c = ec.table_case()
    out, cnt, _pl = ec.snp_model("table")
    assert out["snpmatrix.txt"] == ec.table_expected()
    assert cnt["cells"] == ec.N_TABLE_CELLS >= 5000 and cnt["total_count"] == cnt["kept"] == ec.N_TABLE_CELLS
    assert cnt["hits"] == ec.N_TABLE_CELLS + c["n_unlisted"]
    assert set(_matrix_counts(out["snpmatrix.txt"])) == {1}
    tsize = 2
    while tsize < 2 * ec.N_TABLE_CELLS + 2:                                       # smi_snp_create's table size
        tsize <<= 1
    assert tsize == 16384 and 2 * (ec.N_TABLE_CELLS + 1) + 2 > tsize              # the fullest table: one more cell doubles it
    names = ec.table_names()
    assert "" in names and sum(any(o != n and o.startswith(n) for o in ("N10", "N100", "N1000")) for n in ("N1", "N10", "N100")) == 3
    _t, _r, recs = bammodel.parse_bam(c["bam"])
    bcs = [r["aux"][3:r["aux"].index(b"\0")].decode() for r in recs]
    assert "-1" in bcs and any(b.endswith("-1") and b.count("-1") == 1 for b in bcs) and any(b.count("-1") == 2 for b in bcs)
    assert any(b.startswith("-1N") for b in bcs) and any("-1" in b[1:-2] and not b.endswith("-1") for b in bcs)


# ---- (c) -------------------------------------------------------------------------------------------------------------------------------
def test_walk_case_reaches_the_round_borders():
    c = ec.walk_case()
    _t, _r, recs = bammodel.parse_bam(c["bam"])
    n_ops = sorted(len(r["cigar"]) for r in recs if r["name"].startswith("w"))
    assert n_ops == sorted(ec.WALK_OPS) and max(n_ops) >= 129
    for r in recs:
        if len(r["cigar"]) >= 127:
            assert {op for op, _n in r["cigar"]} >= set("M=XIDNP"), r["name"]
    assert {op for r in recs for op, _n in r["cigar"]} == set("M=XIDNSHP")
    lines = {ln["gene"]: ln for ln in c["lines"]}
    for n in (65, 127, 128, 129, 300):
        for k in (62, 63, 64, 65):
            if k < n:
                for which in ("first", "last"):
                    ln = lines[f"w{n}_op{k}_{which}"]
                    assert ln["ops"] == (k,) and (ln["ok"] or (k == n - 1 and which == "last"))
    assert not lines["w64_op63_last"]["ok"] and lines["w64_op63_first"]["ok"]       # operation 63 ends the read: its last base is refused
    for n, at in ((129, 63), (300, 127)):
        for g in "IDN":
            assert lines[f"after{g}{n}_first"]["ok"] and lines[f"after{g}{n}_first"]["ops"] == (at + 1,) and lines[f"after{g}{n}_both"]["ok"]
    big = next(r for r in recs if r["name"] == "bign")
    assert max(n for op, n in big["cigar"] if op == "N") >= 1 << 27 and [op for op, _n in big["cigar"]].index("N") < 70
    assert lines["bign_after"]["ok"] and lines["bign_far"]["ok"] and not lines["bign_inside"]["ok"]
    assert int(lines["bign_after"]["pos_text"]) > 50_000_000 + (1 << 27)
    assert not lines["plain_lastbase"]["ok"] and lines["plain_before_last"]["ok"]
    assert not lines["clip_under"]["ok"] and not lines["clip_under_and_in"]["ok"] and not lines["clip_before"]["ok"] and lines["clip_first"]["ok"]
    assert sum(g.endswith("_all") and ln["ok"] and len(set(ln["ops"])) > 3 for g, ln in lines.items()) == len(ec.WALK_OPS) - 1
    assert any(g.endswith("_lastdel") for g in lines) and not any(ln["ok"] for g, ln in lines.items() if "_lastdel" in g or "_inD" in g or "_inN" in g)
    assert sum("_inD" in g for g in lines) > 5 and sum("_inN" in g for g in lines) > 5
    # every base code at an even and at an odd read offset on both strands; the reverse strand knows A C G T only
    for strand in "fr":
        got = {}
        for i in list(range(16)) + list(range(17, 33)):
            ln = lines[f"code{strand}{i}"]
            assert ln["ok"]
            got.setdefault(i % 2, []).append(ln["bases"])
        assert set(got[0]) == set(got[1]) == (set("=ACMGRSVTWYHKDBN") if strand == "f" else set("TGCA") | {""})
        assert got[0].count("") == got[1].count("") == (0 if strand == "f" else 12)
    assert {ln["quals"][0] for g, ln in lines.items() if g.startswith("q") and len(ln["quals"]) == 1} == {0, 1, 99, 100, 101, 254}
    types = {g.split("_")[1] for g in lines if g.startswith("rn_")}
    assert types == set("cCsSiI")
    assert {ln["rn"] for g, ln in lines.items() if g.startswith("rn_")} >= {0, -5, 127, 128, 32767, 32768, -32768, 2 ** 31 - 1}
    assert lines["twice"]["rn"] == 9 and lines["twice"]["bc"] == "TWICE"


def test_walk_case_bases_and_qualities_by_construction_equal_the_model():
    c = ec.walk_case()
    for min_rn, min_qv in ec.WALK_FILTERS:
        out, cnt, per_line = ec.snp_model("walk", min_rn=min_rn, min_qv=min_qv)
        counts, mol, rows = ec.walk_expected(min_rn, min_qv)
        assert per_line == counts
        if not rows:                                                              # MINQV above 100 refuses everything: no file
            assert out == {} and min_qv > 100
            continue
        assert out["snpmolinfos.txt"] == mol
        assert [ln.rsplit("\t", cnt["cells"])[0] for ln in out["snpmatrix.txt"].decode().split("\n")[1:-1]] == [r + "\tna" for r in rows]
        assert cnt["rows"] == len(rows) == cnt["kept"]
    assert len(c["lines"]) > 300


def _status(min_rn, min_qv):
    """{line name: "hit" / "lowRN" / "lowQV" / None} as the model counts walk_case under the two filters"""
    _out, _cnt, per_line = ec.snp_model("walk", min_rn=min_rn, min_qv=min_qv)
    return {p["line"].split(",")[3]: next((k for k, v in (("hit", p["hits"]), ("lowRN", p["lowRN"]), ("lowQV", p["lowQV"])) if v), None) for p in per_line}


def test_walk_case_filters_sit_on_both_sides_of_every_quality_and_rn():
    """every (MINRN, MINQV) pair asked for here is one the GPU file runs (ec.WALK_FILTERS)"""
    at = {f: _status(*f) for f in ec.WALK_FILTERS if f[0] == 0 or f[1] == 0}
    for q in (0, 1, 99, 100):                                                     # the quality itself passes, one more refuses it
        assert at[(0, q)][f"q{q}"] == "hit" and at[(0, q + 1)][f"q{q}"] == "lowQV", q
    for q in (101, 254):                                                          # the smallest quality starts at 100
        assert at[(0, 100)][f"q{q}"] == "hit" and at[(0, 101)][f"q{q}"] == "lowQV", q
    assert at[(0, 99)]["q_pair"] == "hit" and at[(0, 100)]["q_pair"] == "lowQV"   # 101 and 99: the smaller one counts
    assert all(at[(0, 254)][f"q{q}"] == at[(0, 255)][f"q{q}"] == "lowQV" for q in (0, 1, 99, 100, 101, 254))
    for name, v in (("rn_C_127", 127), ("rn_c_127", 127), ("rn_C_128", 128), ("rn_s_128", 128), ("rn_s_32767", 32767), ("rn_S_32767", 32767),
                    ("rn_S_32768", 32768), ("rn_i_32768", 32768), ("rn_I_32768", 32768)):
        assert at[(v, 0)][name] == "hit" and at[(v + 1, 0)][name] == "lowRN", name
    assert at[(0, 0)]["rn_c_0"] == at[(0, 0)]["rn_I_0"] == "hit" and at[(1, 0)]["rn_c_0"] == at[(1, 0)]["rn_I_0"] == "lowRN"
    assert at[(0, 0)]["rn_c_-5"] == at[(0, 0)]["rn_s_-32768"] == "lowRN" and at[(-200, 0)]["rn_c_-5"] == at[(-200, 0)]["rn_c_-128"] == "hit"
    assert at[(-200, 0)]["rn_s_-32768"] == "lowRN" and at[(32769, 0)]["rn_S_65535"] == at[(32769, 0)]["rn_i_2147483647"] == "hit"
    assert at[(0, 1)]["q0"] == "lowQV" and _status(128, 100)["q0"] == "lowRN"      # RN is tested first


# ---- (d) -------------------------------------------------------------------------------------------------------------------------------
def _molinfos(out):
    return {(f[0], f[1]): (f[6], f[7], int(f[3])) for f in (ln.split("\t") for ln in out["molinfos.txt"].decode().split("\n")[1:-1])}


def test_iso_case_reaches_its_capacities():
    c = ec.iso_case()
    genes, by_gene, _n = im.parse_refflat(c["refflat"])
    assert [len(by_gene[f"G{n}"]) for n in ec.GENE_SIZES] == list(ec.GENE_SIZES)
    kept, cnt = im.parse_records(c["bam"], dict(cell_tag="BC", umi_tag="U8", gene_tag="GE", rn_tag="RN", max_clip=150, mapqv0=False))
    mols = im.molecules(kept, cnt)
    keys = list(mols)
    n_t = {k: sum(len(by_gene[g]) for g in m["genes"] if g in by_gene) for k, m in mols.items()}
    n_rec = {k: sum(len(r) for r in m["reads"]) for k, m in mols.items()}
    assert {k: n_t[f"{k[0]}:{k[1]}"] for k in c["n_t"]} == c["n_t"] and {k: n_rec[f"{k[0]}:{k[1]}"] for k in c["n_rec"]} == c["n_rec"]
    # nT == lds_tx and nT == lds_tx + 1 are molecules 0 and 1: one block of four waves holds both
    assert keys[:2] == ["S000:lds", "S000:spill"] and (n_t[keys[0]], n_t[keys[1]]) == (ec.LDS_TX, ec.LDS_TX + 1)
    assert set(n_rec.values()) >= {1, 2, 3, 63, 64, 65, 200} and set(n_t.values()) >= {1, 63, 64, 65, 200}
    assert max(a * b for a, b in zip(n_rec.values(), n_t.values())) == 200 * 200
    assert {len(k["junc"]) for k in kept} >= {0, 1, 2, 63, 64, 65}
    assert by_gene["GT"][100][0] == "A000" and min(t + "|GT" for t, _j, _e in by_gene["GT"]) == "A000|GT" and len({str(j) for _t, j, _e in by_gene["GT"]}) == 1
    assert len(mols["S005:nomatch70"]["genes"]) == 70


def test_iso_case_assignments_by_construction_equal_the_model():
    c = ec.iso_case()
    out, cnt = ec.iso_model()
    got = _molinfos(out)
    assert {k: got[k] for k in c["expect"]} == c["expect"]
    assert cnt["ambiguous"] == 2 and cnt["nomatch"] == 5 and cnt["monoexon"] == 1
    gm = out["genematrix.txt"].decode().split("\n")
    assert gm[0] == "geneId" + "".join("\t" + x for x in c["cells"])
    row = ec.gene_matrix_row(c["cells"])
    assert row in out["genematrix.txt"].decode() + "\n" and max(int(v) for v in row.split("\t")[1:]) >= 1000
    at = c["cells"].index("K063")
    assert at == 63 and row.strip().split("\t")[1 + at:3 + at] == ["10", "101"] and row.endswith("\t0\n")   # two widths over cells 63 | 64
    # delta 0 loses the reads that are one or two bases off; a delta larger than the introns matches everything of the right length
    d0 = _molinfos(ec.iso_model(0)[0])
    assert d0[("S007", "off1")] == ("G63", "undef", 0) and d0[("S001", "r63")][1] == "undef" and d0[("S000", "spill")] == got[("S000", "spill")]
    big = _molinfos(ec.iso_model(6000)[0])
    assert big[("S002", "r200")] == ("G200", "G200T000", 200) and ec.iso_model(6000)[1]["ambiguous"] > 8
