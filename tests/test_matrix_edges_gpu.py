"""K-MTX, K-SNP and K-ISO on the edges of their loops, through the file-to-file entry points, every output file byte for byte and every
counter against tests/snpmodel.py / tests/isoformmodel.py and, where the case is built so that the answer is known without the model,
against that answer too.  The inputs are tests/edgecases.py's; tests/test_matrix_edges_cpu.py shows that each of them reaches its edge.

What the seeded runs of tests/test_snp_gpu.py and tests/test_isoform_gpu.py reach (measured with the models): SNPMatrix -- at most 6
candidate lines per record, lines under 120 bases wide, at most 12 CIGAR operations, a largest count of 4, 50 cells.  IsoformMatrix
(_seeded(50000, 7) on the chr12 refFlat) -- 49,472 molecules of 1 to 3 records, candidate sets nT of at most 54 lines (nR * nT at most
162), no molecule anywhere near lds_tx = 2048 (the lds_tx = 2 run has molecules of 2 and of 3 lines, but nothing shows they share a
block), reads of at most 54 junctions, largest counts 7 (isoforms), 8 (genes) and 6 (junctions) in 151 cells.

Trip counts and capacities of K-ISO (smi_isoform.hip, k_iso): one wavefront per molecule; nT = the lines of all its model genes, summed
by one lane-uniform loop over the genes; the counters cnt[0 .. nT) are zeroed 64 per trip, in LDS (2048 per wave) when nT <= lds_tx, in
an HBM slice when nT > lds_tx; the match loop runs over p < nR * nT (64-bit), 64 pairs per trip, each pair finding its line by a walk
over the genes (tx_of) and testing nt * nr junction pairs; best and tied are reduced over nT, 64 per trip; the nomatch gene is a
lane-uniform loop over the genes; the junction set tests the unique junctions of every gene u0 .. u1, 64 per trip, against all j1 - j0
junctions of the molecule, with a ballot per trip."""
import importlib
import os

import pytest

import bammodel
import edgecases as ec

pytestmark = pytest.mark.gpu
SNP_FILES = ("snpmatrix.txt", "snpmetrics.txt", "snpmolinfos.txt")


@pytest.fixture(scope="module")
def snp(pkg):
    return importlib.import_module("sicelore_amd.snpmatrix")


@pytest.fixture(scope="module")
def iso(pkg):
    return importlib.import_module("sicelore_amd.isoformmatrix")


def _run(snp, ctx, tmp_path, case, csv=None, block=0xFF00, segment_bytes=1 << 20, **kw):
    c = ec.SNP_CASES[case]()
    csv_text = c["csv"] if csv is None else csv
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(c["bam"], block=block))
    (tmp_path / "s.csv").write_text(c["snp"])
    (tmp_path / "c.csv").write_text(csv_text)
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    info = snp.snp_matrix(ctx, str(tmp_path / "in.bam"), str(tmp_path / "c.csv"), str(tmp_path / "s.csv"), str(out), prefix="t",
                          segment_bytes=segment_bytes, n_threads=3, **kw)
    want, cnt, per_line = ec.snp_model(case, csv=csv, **{k: v for k, v in kw.items() if k in ("min_rn", "min_qv")})
    assert sorted(os.listdir(out)) == sorted(f"t_{n}" for n in want)
    for name, data in want.items():
        assert (out / f"t_{name}").read_bytes() == data, name
    assert {k: info[k] for k in cnt} == cnt
    assert info["line_counts"] == per_line
    return info, out


# ---- (a) the renderer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cells,zz", [(1, True), (63, True), (64, True), (65, True), (128, True), (129, True), (200, True), (201, True),
                                        (64, False), (65, False), (200, False)])
def test_render_counts_of_one_to_four_digits_in_n_cells(snp, gpu_ctx, tmp_path, n_cells, zz):
    """0, 1, 9, 10, 11, 99, 100, 101, 999, 1000, 1001 distinct UMIs per (row, cell), 1 to 3 records each with the repeats in later
    segments, side by side over cells 63 | 64 and 127 | 128; zz: a listed cell without a hit in the last column, and hit cells not
    listed (201 lists them all: the row hit only in C199 appears); without zz the last column, in front of the line feed, holds counts"""
    info, out = _run(snp, gpu_ctx, tmp_path, "render", csv=ec.render_csv(n_cells, zz), segment_bytes=40000)
    mat, met, labels = ec.render_expected(n_cells, zz)
    assert (out / "t_snpmatrix.txt").read_bytes() == mat and (out / "t_snpmetrics.txt").read_bytes() == met
    assert info["rows"] == len(labels) and info["render_blocks"] == 1


@pytest.mark.parametrize("budget", ["around", "before_only", "after_only", "none", "less_than_a_row"])
def test_render_block_breaks_around_the_widest_row(snp, gpu_ctx, tmp_path, budget):
    """five rows of 201 cells, row 1 holds the widest count (1001) and row 0 a longer label: budgets that break directly in front of
    row 1 and behind it, only in front of it, only behind it, at neither place; under one smaller than a row matrix() renders one row
    per block"""
    mat, met, labels = ec.render_expected(201)
    nbytes, blocks = ec.render_budgets()[budget]
    info, out = _run(snp, gpu_ctx, tmp_path, "render", csv=ec.render_csv(201), budget_bytes=nbytes)
    assert (out / "t_snpmatrix.txt").read_bytes() == mat
    assert info["render_blocks"] == len(ec.render_blocks(labels, 201, 1001, nbytes)) == len(blocks)


def test_render_a_count_of_100003_and_every_width_up_to_six_digits(snp, gpu_ctx, tmp_path):
    info, out = _run(snp, gpu_ctx, tmp_path, "wide", segment_bytes=200000)
    mat, met, _labels = ec.wide_expected()
    assert (out / "t_snpmatrix.txt").read_bytes() == mat and (out / "t_snpmetrics.txt").read_bytes() == met
    assert b"\t100003\t0\t10\n" in mat and info["total_count"] == sum(ec.WIDE_COUNTS.values())


# ---- (b) the candidate search ----------------------------------------------------------------------------------------------------------
def test_search_batches_borders_and_the_running_maximum(snp, gpu_ctx, tmp_path):
    """records under 0, 1, 63, 64, 65, 128 and 200 lines of their strand, interleaved with lines of the other strand and lines that end
    one base in front of them; inclusive borders; a wide line sorted in front of 400 short ones; lines of one first position; a
    reference without lines, one without records, an unmapped record"""
    c = ec.search_case()
    info, out = _run(snp, gpu_ctx, tmp_path, "search", block=3000, segment_bytes=3000)
    assert [(p["line"], p["hits"]) for p in info["line_counts"]] == c["hits"]
    rows = (out / "t_snpmatrix.txt").read_bytes().decode().split("\n")[1:-1]
    assert ["\t".join(r.split("\t")[:3]) for r in rows] == c["rows"] and all(sorted(r.split("\t")[3:])[-2:] == ["0", "1"] for r in rows)


def test_search_looks_at_the_record_only_the_wide_line_reaches(pkg, snp, gpu_ctx, tmp_path):
    """wide_only lies behind every short line and inside `wide`, which cannot resolve on it: that the record was looked at shows only in
    the cast of its attributes -- its RN is a string here (a valid BAM the reference cannot read), and the run has to stop naming it"""
    c = ec.search_case(bad_rn=True)
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(c["bam"]))
    (tmp_path / "s.csv").write_text(c["snp"])
    (tmp_path / "c.csv").write_text(c["csv"])
    with pytest.raises(pkg.SmiError, match="read wide_only: an attribute"):
        snp.snp_matrix(gpu_ctx, str(tmp_path / "in.bam"), str(tmp_path / "c.csv"), str(tmp_path / "s.csv"), str(tmp_path))


def test_cell_table_of_8191_cells_each_hit_once(snp, gpu_ctx, tmp_path):
    """smi_snp_create sizes the table to the smallest power of two >= 2 * cells + 2: 8,191 cells fill 16,384 slots to a load factor of
    0.49994, the fullest it gets.  N1 is a prefix of N10 and N100; the barcodes carry "-1" at the end, in the middle, twice, in front,
    and one is "-1" alone (the empty name); six hit barcodes are not listed"""
    info, out = _run(snp, gpu_ctx, tmp_path, "table", segment_bytes=100000)
    assert (out / "t_snpmatrix.txt").read_bytes() == ec.table_expected()
    assert info["kept"] == ec.N_TABLE_CELLS and info["hits"] == ec.N_TABLE_CELLS + 6


# ---- (c) the CIGAR walk ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_rn,min_qv", ec.WALK_FILTERS)
def test_walk_rounds_bases_qualities_and_rn(snp, gpu_ctx, tmp_path, min_rn, min_qv):
    """CIGARs of 1, 63, 64, 65, 127, 128, 129 and 300 operations of M = X I D N S H P; positions on the first and last base of operations
    62 .. 65, behind an I, a D and an N that end a round, behind an intron of 2^27 bases; the last base of the read; the soft clip; a
    deletion under the last position only; the sixteen base codes at even and odd offsets on both strands; qualities 0 .. 254 and RN of
    every integer type on both sides of MINQV and MINRN; attributes given twice, B arrays and H in front"""
    info, out = _run(snp, gpu_ctx, tmp_path, "walk", block=2000, segment_bytes=2500, min_rn=min_rn, min_qv=min_qv)
    counts, mol, rows = ec.walk_expected(min_rn, min_qv)
    assert info["line_counts"] == counts and info["rows"] == len(rows)
    if rows:
        assert (out / "t_snpmolinfos.txt").read_bytes() == mol
        got = (out / "t_snpmatrix.txt").read_bytes().decode().split("\n")[1:-1]
        assert ["\t".join(r.split("\t")[:2]) for r in got] == rows
    else:
        assert min_qv > 100 and info["bytes_written"] == 0


# ---- (d) K-ISO -------------------------------------------------------------------------------------------------------------------------
def _run_iso(iso, ctx, tmp_path, **kw):
    c = ec.iso_case()
    (tmp_path / "in.bam").write_bytes(bammodel.bgzf_compress(c["bam"], block=3000))
    (tmp_path / "r.refFlat").write_text(c["refflat"])
    (tmp_path / "c.csv").write_text(c["csv"])
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    info = iso.isoform_matrix(ctx, str(tmp_path / "in.bam"), str(tmp_path / "r.refFlat"), str(tmp_path / "c.csv"), str(out), prefix="t",
                              segment_bytes=9000, n_threads=3, **kw)
    want, cnt = ec.iso_model(kw.get("delta", 2), kw.get("isobam", False))
    assert sorted(os.listdir(out)) == sorted([f"t_{n}" for n in want] + ["t.log"])
    for name, data in want.items():
        got = (out / f"t_{name}").read_bytes()
        assert (bammodel.bgzf_decompress(got) if name == "isobam.bam" else got) == data, name
    assert {k: info[k] for k in cnt} == cnt
    return info, out


@pytest.mark.parametrize("lds_tx", [ec.LDS_TX, 1, 2048])
def test_iso_candidate_sets_around_lds_tx(iso, gpu_ctx, tmp_path, lds_tx):
    """molecules of 1, 63, 64, 65 and 200 records on genes of 1, 63, 64, 65 and 200 lines; with lds_tx = 64 molecule 0 (64 lines) stays
    in LDS and molecule 1 (65 lines) spills, both in block 0; ties among 130 lines (the winner is line 100) and among 70 genes; reads
    of 0, 1, 64 and 65 junctions; 1001 molecules in one cell of the gene matrix"""
    c = ec.iso_case()
    info, out = _run_iso(iso, gpu_ctx, tmp_path, lds_tx=lds_tx, isobam=lds_tx == ec.LDS_TX)
    # deliberately two-sided and not exact: a molecule of exactly lds_tx lines may stay in LDS (it does today) or spill -- it computes the
    # same either way, and the molecules 0 and 1 of this case are there to show that.  Fewer spills would run over the LDS.
    n_t = list(c["n_t"].values()) + [1] * (info["molecules"] - len(c["n_t"]))
    assert sum(n > lds_tx for n in n_t) <= info["spill"] <= sum(n >= lds_tx for n in n_t)
    assert lds_tx != 2048 or info["spill"] == 0
    mi = {(f[0], f[1]): (f[6], f[7], int(f[3])) for f in (ln.split("\t") for ln in (out / "t_molinfos.txt").read_bytes().decode().split("\n")[1:-1])}
    assert {k: mi[k] for k in c["expect"]} == c["expect"]
    assert ec.gene_matrix_row(c["cells"]) in (out / "t_genematrix.txt").read_bytes().decode()


@pytest.mark.parametrize("delta", [0, 6000])
def test_iso_delta_zero_and_larger_than_an_intron(iso, gpu_ctx, tmp_path, delta):
    info, _out = _run_iso(iso, gpu_ctx, tmp_path, delta=delta, lds_tx=ec.LDS_TX, budget_bytes=2000)
    assert info["render_blocks"] > 10 and (info["nomatch"] > 5 if delta == 0 else info["ambiguous"] > 8)
