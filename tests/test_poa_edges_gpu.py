"""K-POA (smi_consensus.hip) on the cases of tests/poacases.py, byte for byte against tests/consensusmodel.py: chunk seams, long gaps in the
read and in the graph, ties, wide groups, int16 rows at 30,000 -- and the persistent-wave loop with fewer slots than molecules, asserted
from the library's own launch statistics (smi_poa_batch_ex): a slot is never cleared, so every molecule but the first of a slot runs on
the graph, rows and heap another one left there."""
import importlib

import numpy as np
import pytest

import consensusmodel as cm
import poacases as pc
from test_consensus_gpu import _bam_file, _filters_records, _outgrows_estimate, noisy_molecule

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(pkg):
    return importlib.import_module("sicelore_amd.lib")


@pytest.fixture(scope="module")
def cc(pkg):
    return importlib.import_module("sicelore_amd.computeconsensus")


# the run families twice: on the 400-base source, and on the 200-base one whose cases tests/test_poa_edges_cpu.py shows to notice each mutant
FAMILY_CALLS = [(f, ()) for f in pc.FAMILIES if f != "int16_extreme"] + [("ins_runs", (200,)), ("del_runs", (200,))]


@pytest.mark.parametrize("fam,args", FAMILY_CALLS, ids=[f + "".join(map(str, a)) for f, a in FAMILY_CALLS])
def test_family_in_one_call(lib, gpu_ctx, fam, args):
    mols = list(pc.family(fam, *args).values())
    rerun = pc.check_poa(lib, gpu_ctx, mols)
    if len(mols) == 1:                                              # alone in its launch, its slot is its own estimate: the model says if it overflows
        recs = pc.model_trace(mols[0])[1]
        assert rerun == any(r["nodes"] > 3 * max(map(len, mols[0])) for r in recs)


def test_int16_rows_at_30000(lib, gpu_ctx):
    """6,000 x 6,000 cells in int16 rows, H up to exactly 30,000 (tests/test_poa_edges_cpu.py asserts that figure on the model)"""
    mols = list(pc.family("int16_extreme").values())
    assert pc.check_poa(lib, gpu_ctx, mols) == 0


def test_every_family_shuffled_into_one_call(lib, gpu_ctx):
    mols = [m for f in pc.FAMILIES for m in pc.family(f).values()] + [m for f in ("ins_runs", "del_runs") for m in pc.family(f, 200).values()]
    rng = np.random.default_rng(7)
    mols = [mols[i] for i in rng.permutation(len(mols))]
    _rerun, st = pc.check_poa(lib, gpu_ctx, mols, max_ps=30, stats=True)
    assert st["launches"] >= 3                                      # molecules of very different sizes: several launch groups


def test_plain_call_keeps_its_four_results(lib, gpu_ctx):
    mols = list(pc.family("low_complexity").values())
    assert len(lib.poa_batch(gpu_ctx, *pc.batch(mols))) == 4
    *_four, st = lib.poa_batch(gpu_ctx, *pc.batch(mols), stats=True)
    assert set(st) == {"launches", "waves", "slot_reuse", "max_slot_bytes"} and st["launches"] >= 1 and st["max_slot_bytes"] > 0


def test_slot_reuse_identical_shapes(lib, gpu_ctx):
    """40 molecules of 4 reads x 96 bases are one launch group of one slot size: a budget of one slot runs all 40 in the same slot, one after
    the other; a budget of three runs them on three waves"""
    rng = np.random.default_rng(401)
    mols = []
    for _ in range(40):
        src = cm.random_seq(rng, 96)
        mols.append(tuple(pc.fit(rng, cm.noisy_copy(rng, src, 0.1), 96) for _ in range(4)))
    rerun, free = pc.check_poa(lib, gpu_ctx, mols, stats=True, scratch_bytes=0)
    assert rerun == 0 and free["launches"] == 1 and free["waves"] == 40 and free["slot_reuse"] == 0
    slot = free["max_slot_bytes"]
    rerun, one = pc.check_poa(lib, gpu_ctx, mols, stats=True, scratch_bytes=slot)
    assert (rerun, one["launches"], one["waves"], one["slot_reuse"], one["max_slot_bytes"]) == (0, 1, 1, 39, slot)
    rerun, three = pc.check_poa(lib, gpu_ctx, mols, stats=True, scratch_bytes=3 * slot)
    assert (rerun, three["launches"], three["waves"], three["slot_reuse"], three["max_slot_bytes"]) == (0, 1, 3, 37, slot)


def test_slot_reuse_mixed_shapes(lib, gpu_ctx):
    """60 molecules of 3..8 reads of 30..300 bases; the budget is the largest slot, so the largest molecules share one slot and every smaller
    one runs on the remains of a larger: its graph arrays, DP rows and heap lie inside what the larger one wrote"""
    rng = np.random.default_rng(402)
    wide = pc.family("wide_groups")
    mols = [(b"", b"", b""), (b"A", b"", b"G", b"A"), wide["wide-20"], wide["wide-20-crossed"]]
    while len(mols) < 60:
        mols.append(tuple(noisy_molecule(rng, int(rng.integers(3, 9)), int(rng.integers(30, 301)), 0.1)))
    mols = [mols[i] for i in rng.permutation(60)]
    _rerun, free = pc.check_poa(lib, gpu_ctx, mols, stats=True)
    assert free["slot_reuse"] == 0
    _rerun, st = pc.check_poa(lib, gpu_ctx, mols, stats=True, scratch_bytes=free["max_slot_bytes"])
    assert st["slot_reuse"] >= 30 and st["max_slot_bytes"] == free["max_slot_bytes"]


def test_slot_reuse_across_the_rerun_pass(lib, gpu_ctx):
    """the six molecules of test_poa_graphs_that_outgrow_the_estimate_run_again overflow their first slot and run again in a worst-case slot
    that the one before them has used"""
    rng = np.random.default_rng(104)
    mols = [tuple(cm.random_seq(rng, 100) for _ in range(10)) for _ in range(6)]
    assert all(_outgrows_estimate(m) for m in mols)
    mols += [tuple(noisy_molecule(rng, int(rng.integers(3, 6)), int(rng.integers(30, 61)))) for _ in range(20)]
    rerun, free = pc.check_poa(lib, gpu_ctx, mols, stats=True)
    assert rerun == 6
    rerun, st = pc.check_poa(lib, gpu_ctx, mols, stats=True, scratch_bytes=free["max_slot_bytes"])
    assert rerun == 6 and st["slot_reuse"] > 0 and st["launches"] >= 2


def test_file_path_reuses_slots(cc, lib, gpu_ctx, tmp_path):
    """ComputeConsensus hands K-POA all its molecules in one batch; with the scratch budget of one slot (the size from smi_poa_batch_ex on
    the same molecules) they follow each other through it and the FASTQ is still the model's"""
    recs = _filters_records(np.random.default_rng(201))
    bam, path = _bam_file(tmp_path, recs, block=5000)
    cfg = dict(cm.DEFAULTS)
    kept, cnt = cm.parse_records(bam, cfg)
    mols = [sel for _name, sel in cm.molecules(kept, cfg["max_reads"], cnt) if len(sel) >= 3]
    *_four, st = lib.poa_batch(gpu_ctx, *pc.batch(mols), stats=True)
    info = cc.compute_consensus(gpu_ctx, str(path), str(tmp_path / "out.fq"), segment_bytes=20000, scratch_bytes=st["max_slot_bytes"])
    want, cnt = cm.compute_consensus(bam)
    assert (tmp_path / "out.fq").read_bytes() == want
    assert info["poa_molecules"] == len(mols) > 5
    assert info["poa_slot_reuse"] > 0 and info["poa_launches"] >= 1 and info["poa_rerun"] == 0
    plain = cc.compute_consensus(gpu_ctx, str(path), str(tmp_path / "plain.fq"), segment_bytes=20000)
    assert plain["poa_slot_reuse"] == 0 and (tmp_path / "plain.fq").read_bytes() == want
