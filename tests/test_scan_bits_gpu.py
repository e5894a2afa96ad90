"""K-SCAN's phase A on 32-bit words and three-input operations, in the kernels: the ends tests/test_scan_bits_cpu.py builds and proves (polyT entries
whose bases lie across every 32-bit seam of the finder's words, entries at positions 0 and 149, counts exactly at and one below the thresholds
12 and 10 of 15 and 3 of 5, walks back decided across the halves of the 64-bit window, pairs of TSO candidates at distance 26 and 27 across positions
63 / 64 / 65, ending at 90 and starting at 1) in batches of 1, 33 and 65 reads -- one tile, a second tile with two lanes, a third with two -- with the
end under test at lane 0, at lane 63 and on the last read: the shipped kernels (the bit-sliced masks) and the generic ones (the loop finder, every TSO
candidate aligned) against the oracle in passes 2 and 1, whole records, then the record fields the catalogue names."""
import numpy as np
import pytest

from test_scan_bits_cpu import NAMES, SIZES, TSO_PAIRS, check_polyt_records, check_tso_records, polyt_batch, tso_batch
from test_scan_lanes_gpu import _batch, _run_all

pytestmark = pytest.mark.gpu

GROUPS = [NAMES[i:i + 10] for i in range(0, len(NAMES), 10)]
TSO_GROUPS = [sorted(TSO_PAIRS)[i:i + 8] for i in range(0, len(TSO_PAIRS), 8)]


@pytest.mark.parametrize("group", range(len(GROUPS)))
@pytest.mark.parametrize("n", SIZES)
def test_polyt_seams_in_batches(pkg, sor, gpu_ctx, monkeypatch, n, group):
    for j, name in enumerate(GROUPS[group]):
        k = 10 * group + j
        ends, where = polyt_batch(n, name, k)
        ra, qa, offs = _batch(ends, np.random.default_rng(9600 + 37 * n + k))
        exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)        # shipped == generic == oracle, passes 2 and 1
        check_polyt_records(exp, offs, where)


@pytest.mark.parametrize("group", range(len(TSO_GROUPS)))
@pytest.mark.parametrize("n", SIZES)
def test_tso_pairs_in_batches(pkg, sor, gpu_ctx, monkeypatch, n, group):
    for j, name in enumerate(TSO_GROUPS[group]):
        ends, where = tso_batch(n, name)
        ra, qa, offs = _batch(ends, np.random.default_rng(9700 + 37 * n + 8 * group + j))
        exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
        check_tso_records(exp, where)
