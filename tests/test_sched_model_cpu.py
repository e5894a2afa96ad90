"""tools/sched_model.py's simulator on work whose answer is hand arithmetic: equal work leaves no idle slot apart from the tail under any of the three
policies, and one slow wave per block costs the block policy its siblings' waiting time and the other two nothing but the tail."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sched_model as sm  # noqa: E402


def test_equal_work_idles_only_in_the_tail():
    # 40 units of 3 on 16 slots: two full turns and a third with 8 units
    costs = np.full(40, 3.0)
    for policy in ("blocks", "waves", "claim"):
        r = sm.simulate(costs, 16, policy)
        assert r["idle_inner"] == 0.0, policy
        assert r["makespan"] == 9.0 and r["busy"] == 120.0, policy
        assert r["idle_tail"] == r["idle"] == 16 * 9.0 - 120.0, policy
    # work that fills the slots exactly: no tail either
    for policy in ("blocks", "waves", "claim"):
        r = sm.simulate(np.full(32, 3.0), 16, policy)
        assert r["idle"] == 0.0 and r["makespan"] == 6.0, policy
    # a block that strides over tiles (a grid of 4 blocks for 8 block-tiles) is the same when the work is equal
    r = sm.simulate(np.full(32, 3.0), 16, "blocks", grid_blocks=4)
    assert r["idle"] == 0.0 and r["makespan"] == 6.0


def test_one_slow_wave_per_block():
    # four blocks of [10, 1, 1, 1] on 8 slots = 2 block slots
    costs = np.tile([10.0, 1.0, 1.0, 1.0], 4)
    a = sm.simulate(costs, 8, "blocks")
    # a block lasts 10; each block slot runs two: 20.  Its three fast waves wait 9 each: 27 per block, 108 in all; both block slots end together
    assert a["makespan"] == 20.0 and a["idle_inner"] == 108.0 and a["idle_tail"] == 0.0
    assert a["idle"] == 8 * 20.0 - 52.0
    for policy in ("waves", "claim"):
        c = sm.simulate(costs, 8, policy)
        assert c["idle_inner"] == 0.0 and c["idle"] == c["idle_tail"], policy
        # in order on 8 slots: the slow units start at 0, 0, 1 and 1 (the third and fourth behind a unit of 1), so the launch ends at 11
        assert c["makespan"] == 11.0 and c["idle"] == 8 * 11.0 - 52.0, policy
    # the grid-stride form: 2 blocks, each two block-tiles; wave 0 of a block has 20, the others 2: 3 x 18 wait per block
    s = sm.simulate(costs, 8, "blocks", grid_blocks=2)
    assert s["makespan"] == 20.0 and s["idle_inner"] == 2 * 3 * 18.0 and s["idle_tail"] == 0.0


def test_unit_overhead_counts_as_work():
    r = sm.simulate(np.full(16, 3.0), 16, "waves", unit_overhead=1.0)
    assert r["makespan"] == 4.0 and r["busy"] == 64.0 and r["idle"] == 0.0
