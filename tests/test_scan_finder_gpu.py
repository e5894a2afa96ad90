"""The tail of the bit-parallel polyT finder as mask operations, and the adapter tie key from the table, in the kernels: the ends
tests/test_scan_finder_cpu.py builds and proves (PLANTS: advances of `start` at the strides' and the registers' edges, probe holes a stride jumps, runs
that reach and pass the window, entries at 0 and 149, forward steps that stop at n - 1, N inside a run) in batches of 1, 33, 65 and 129 reads -- one
partly filled wave, a second wave with two lanes, a wave seam, a block seam -- with the end under test at lane 0, at lane 63 and on the
reverse-complemented tail of the last read: the shipped kernels (the masks) and the generic ones (the loop) against the oracle in passes 2 and 1, whole
records."""
import numpy as np
import pytest

from test_scan_finder_cpu import MORE_TIES, PLANTS, WINDOW, c_end, codes_of, fm
from test_scan_lanes_gpu import F_A3, F_T5, _batch, _run_all
from test_scan_lazy_cpu import AD_POS, tie_end

pytestmark = pytest.mark.gpu

NAMES = sorted(PLANTS)


def _end1(name):
    T, G, first = fm.masks_of(codes_of(PLANTS[name][0]))
    return fm.tail_loops(T, G, first, WINDOW)[2]


def _plant_batch(n, k):
    """n reads: plant k on read 0's head (lane 0), on the tail of read 31 (lane 63) and on the last read's tail; every other read carries another plant
    on alternating sides.  -> [(head, tail)], {read: name}"""
    ends, where = [], {}
    for i in range(n):
        name = NAMES[(k + i) % len(NAMES)]
        side = i % 2
        if i == 0:
            name, side = NAMES[k], 0
        if i == 31 or i == n - 1:
            name, side = NAMES[k], (1 if n > 1 else 0)
        own = list(PLANTS[name][0])
        ends.append((own, c_end()) if side == 0 else (c_end(), own))
        where[i] = name
    return ends, where


def _pe(exp, offs):
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    return np.where(exp["polya_start"] != 0, lens - exp["polya_start"] + 1, 0)   # K-SCAN: polya_start = len - (pe - 1) once a side is chosen


@pytest.mark.parametrize("n", [1, 33, 65, 129])
def test_plants_in_batches(pkg, sor, gpu_ctx, monkeypatch, n):
    want = {name: _end1(name) for name in NAMES}
    for k in range(len(NAMES)):
        ends, where = _plant_batch(n, k)
        ra, qa, offs = _batch(ends, np.random.default_rng(8100 + 37 * n + k))
        exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
        pe = _pe(exp, offs)
        # the oracle ends every run where the CPU model of the tail does (entry_at_0 has no room for an adapter in front of it: its record shows the flag alone)
        assert pe.tolist() == [0 if where[i] == "entry_at_0" else want[where[i]] for i in range(n)], (n, k)
        assert ((exp["flags"].astype(np.int64) & (F_T5 | F_A3)) != 0).all()


def test_one_read_plant_on_the_tail(pkg, sor, gpu_ctx, monkeypatch):
    """a single read whose reverse-complemented tail carries the plant: lane 1 of a wave with two active lanes"""
    for name in NAMES:
        ra, qa, offs = _batch([(c_end(), list(PLANTS[name][0]))], np.random.default_rng(8200))
        exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
        assert _pe(exp, offs).tolist() == [0 if name == "entry_at_0" else _end1(name)] and int(exp["flags"][0]) & F_A3


def test_polyt_on_both_ends(pkg, sor, gpu_ctx, monkeypatch):
    """reads with a polyT on BOTH ends (none among the generator's reads): the wave takes the other gate path, and both lanes of a pair run the tail"""
    ends = []
    for i in range(33):
        a, b = list(PLANTS[NAMES[i % len(NAMES)]][0]), list(PLANTS[NAMES[(i + 7) % len(NAMES)]][0])
        ends.append((a, b) if i % 3 == 0 else ((a, c_end()) if i % 3 == 1 else (c_end(), b)))
    ra, qa, offs = _batch(ends, np.random.default_rng(8301))
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
    both = 1 << 14                                   # SMI_F_POLY_T_5P_POLY_A_3P
    assert ((exp["flags"].astype(np.int64) & both) != 0).sum() == 11


def test_n_inside_the_run(pkg, sor, gpu_ctx, monkeypatch):
    """exact T excludes N: every lane of a wave and two more carry a run with N in it"""
    ends = []
    for i in range(34):
        own = list(PLANTS["n_inside_the_run" if i % 2 else "n_ends_the_run"][0])
        ends.append((own, c_end()) if i % 4 < 2 else (c_end(), own))
    ra, qa, offs = _batch(ends, np.random.default_rng(8401))
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
    assert set(_pe(exp, offs).tolist()) == {_end1("n_inside_the_run"), _end1("n_ends_the_run")} and _end1("n_ends_the_run") == 60


def test_ties_on_k12_and_on_k10(pkg, sor, gpu_ctx, monkeypatch):
    """adapter ties whose keys differ in k12 alone and in k10 alone, two error columns on one side (test_scan_finder_cpu.test_more_adapter_ties proves them)"""
    ends, plan = [], []
    for i in range(32):
        slices, win = MORE_TIES[i % len(MORE_TIES)]
        own = tie_end(slices)
        ends.append((own, c_end()) if i % 2 == 0 else (c_end(), own))
        plan.append(win)
    ra, qa, offs = _batch(ends, np.random.default_rng(8501))
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    assert exp["adapter_found"].sum() == 32
    assert (lens - exp["adapter_start"] + 1).tolist() == [AD_POS[w] for w in plan]
