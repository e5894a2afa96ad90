#!/usr/bin/env python3
"""What it costs K-SCAN and K-BC1 that their waves get work by the block: a CPU model of three ways to put the waves of a launch on the wave slots of
an MI355X (1,024 SIMDs; K-SCAN holds 4 waves per SIMD, K-BC1 8).

  (a) blocks   blocks of four independent waves; a block's four slots are freed when its slowest wave is done.  K-SCAN: a grid of 64 blocks per CU,
               a block strides over tiles of 256 ends (a wave over its 64 of each); K-BC1: one batch of 64 reads per wave, a block per four batches
  (b) waves    units of one wave (one tile of 64 ends / one batch) handed out by the hardware in order, a slot freed per wave
  (c) claim    as many waves as there are slots; a wave takes its next unit from the counter of one of sixteen ranges when it has finished one

Per-wave work of K-SCAN comes from the CPU models of the bench generator's reads: the 4-mer gates of tools/scan_gate_model.py give a wave's adapter
and TSO candidates, hence its alignment rounds and whether the isolated-candidate pre-filter runs; the shares of waves that enter the tie branch and
the second alignment of a rescue come from the outputs of tools/scan_lazy_model.py and tools/scan_rescue_model.py (drawn per wave at those shares).
The regions are priced with the per-wave VALU figures of DESIGN.md section 10 (fills ~ 980, walks and folds ~ 470, finder ~ 570, TSO gates and
pre-filter 857, the rest ~ 480 of 3,356).  K-BC1's per-wave work is its look-up rounds (pairs per 64 reads / 64) and the second-bucket walk of one
wave in nine; the pairs are DRAWN to the mean the kernel's comment gives (~ 102 per wave), not derived from reads.

A wave's time is its work and nothing else: see "leaves_out" in the output.  No GPU needed.
usage: sched_model.py [sample waves] [out.json]"""
import heapq
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SIMD = 1024
AD10 = "CTTCCGATCT"
# VALU instructions per wave by region, K-SCAN <10, 3', shipped>
REGION = {"fills": 980.0, "walks_folds": 470.0, "finder": 570.0, "tso_gates_prefilter": 857.0, "rest": 480.0}
PREFILTER_SHARE = 0.25   # of tso_gates_prefilter: the pre-filter's part, paid by the waves in which it can save a round
TIE_VALU = 120.0         # two nw_end5 of a tie ("~ 110 of them")


def simulate(costs, n_slots, policy, block_waves=4, grid_blocks=None, unit_overhead=0.0, shards=16):
    """costs[u]: time of work unit u (one wave's tile or batch), in any unit -> dict of makespan, busy, idle, idle_inner, idle_tail (slot x time).
    policy "blocks": n_slots / block_waves block slots take blocks in order; block b of a grid of grid_blocks (default: one block-tile each) owns
    the units block_waves * t + w of its block-tiles t = b, b + grid_blocks, ...; a block lasts as long as its slowest wave.  idle_inner = the
    slots of finished waves waiting for their block, idle_tail = block slots empty before the launch ends.
    policy "waves": every slot takes the next unit in order when it is free; policy "claim": a slot takes the next unit of its shard's range, then
    of the next range with units left (idle_inner is 0 by construction in both); unit_overhead is added to every unit (the start of a one-wave
    block / a claim on the wave's critical path)."""
    costs = np.asarray(costs, dtype=np.float64)
    n = costs.size
    busy = float(costs.sum())
    if policy == "blocks":
        n_tiles = (n + block_waves - 1) // block_waves
        padded = np.zeros(n_tiles * block_waves)
        padded[:n] = costs
        padded = padded.reshape(n_tiles, block_waves)
        g = n_tiles if grid_blocks is None else min(grid_blocks, n_tiles)
        per_wave = np.zeros((g, block_waves))
        for b0 in range(0, n_tiles, g):
            part = padded[b0:b0 + g]
            per_wave[:part.shape[0]] += part
        dur = per_wave.max(1)
        slots = [0.0] * min(n_slots // block_waves, g)
        heapq.heapify(slots)
        for d in dur:
            heapq.heapreplace(slots, slots[0] + d)
        makespan = max(slots)
        used = len(slots) * block_waves
        inner = float((block_waves * dur - per_wave.sum(1)).sum())
        tail = float(sum(makespan - t for t in slots)) * block_waves + (n_slots - used) * makespan
    elif policy == "claim":
        # K-SCAN's scheme (smi_wave.h WaveClaim): the units cut into `shards` consecutive ranges; a slot takes from the range of its shard and, when
        # that has run out, from the next range that has units left
        per = (n + shards - 1) // shards
        head = [min(s * per, n) for s in range(shards)]
        end = [min((s + 1) * per, n) for s in range(shards)]
        heap = [(0.0, k) for k in range(min(n_slots, n))]
        home = {k: k % shards for _, k in heap}
        finish = []
        left = n
        while left:
            t, k = heapq.heappop(heap)
            s = home[k]
            while head[s] >= end[s]:
                s = (s + 1) % shards
            home[k] = s
            heapq.heappush(heap, (t + costs[head[s]] + unit_overhead, k))
            head[s] += 1
            left -= 1
        finish = [t for t, _ in heap]
        makespan = max(finish)
        busy += unit_overhead * n
        inner = 0.0
        tail = float(sum(makespan - t for t in finish)) + (n_slots - len(finish)) * makespan
    else:
        slots = [0.0] * min(n_slots, n)
        heapq.heapify(slots)
        for c in costs:
            heapq.heapreplace(slots, slots[0] + c + unit_overhead)
        makespan = max(slots)
        busy += unit_overhead * n
        inner = 0.0
        tail = float(sum(makespan - t for t in slots)) + (n_slots - len(slots)) * makespan
    return {"makespan": float(makespan), "busy": busy, "idle": inner + tail, "idle_inner": inner, "idle_tail": tail,
            "idle_share_of_slot_time": (inner + tail) / (n_slots * makespan) if makespan else 0.0}


def _share(path, key, default):
    try:
        return float(json.load(open(os.path.join(ROOT, path)))[key])
    except (OSError, KeyError, ValueError):
        return default


def scan_wave_costs(sample_waves, rng):
    """VALU instructions of sample_waves waves of the timed step's reads -> (costs, description of the sample)"""
    import scan_gate_model as gm

    graft = gm.graft
    synth = importlib.import_module(graft.load_package().__name__ + ".synth")
    sor = graft.load_oracle()
    sor.build()
    wl = synth.make_whitelist(200_000, seed=1, device="cpu")
    used = synth.pick_used(wl, 5000, seed=2)
    rd = synth.gen_reads(32 * sample_waves, used, seed=1000, device="cpu")   # the timed step's generator call (bench.py: seed 1000 + chunk)
    ends = gm.scan_ends(rd)
    tm = gm.gate_masks(ends, gm.TSO, gm.TSO_WINDOW)
    iso = gm.isolated(tm)
    am = gm.gate_masks(ends, AD10, ends.shape[1])
    n_ad = np.zeros(ends.shape[0], dtype=np.int64)
    for e in range(ends.shape[0]):
        bt = sor.find_polyt(ends[e].astype(np.uint8))
        if bt is not None:
            n_ad[e] = int(am[e][:max(bt[1] - 12, 0)].sum())
    rounds = lambda x: (x + 63) // 64  # noqa: E731
    ad_tot = n_ad.reshape(sample_waves, 64).sum(1)
    tso_tot = tm.reshape(sample_waves, 64, -1).sum((1, 2))
    tso_iso = iso.reshape(sample_waves, 64, -1).sum((1, 2))
    prefilter = rounds(tso_tot) > rounds(tso_tot - tso_iso)          # the pre-filter runs where it can save a round ...
    tso_rounds = np.where(prefilter, rounds(tso_tot - tso_iso), rounds(tso_tot))   # ... and is taken to save it (it drops isolated candidates only)
    ad_rounds = rounds(ad_tot)
    p_tie = _share("profiles/scan_lazy/lazy_model.json", "share_of_waves_entering_the_tie_branch", 0.4944)
    p_rescue = _share("profiles/scan_tso_counts/rescue_model.json", "share_of_waves_with_such_an_end", 0.032)
    tie = rng.random(sample_waves) < p_tie
    rescue = rng.random(sample_waves) < p_rescue
    n_rounds = ad_rounds + tso_rounds + rescue                       # a rescue aligns the winners again: one more round
    per_round = (REGION["fills"] + REGION["walks_folds"]) / max(float(n_rounds.mean()), 1e-9)
    gates = REGION["tso_gates_prefilter"] * (1.0 - PREFILTER_SHARE)
    pre = REGION["tso_gates_prefilter"] * PREFILTER_SHARE / max(float(prefilter.mean()), 1e-9)
    rest = REGION["rest"] - TIE_VALU * p_tie
    costs = rest + REGION["finder"] + gates + pre * prefilter + per_round * n_rounds + TIE_VALU * tie
    info = {"sample_waves": sample_waves, "adapter_rounds_mean": float(ad_rounds.mean()), "tso_rounds_mean": float(tso_rounds.mean()),
            "share_of_waves_with_two_or_more_tso_rounds": float((tso_rounds >= 2).mean()), "share_of_waves_prefilter_runs": float(prefilter.mean()),
            "share_tie": p_tie, "share_rescue": p_rescue, "valu_per_round": per_round, "valu_per_wave_mean": float(costs.mean()),
            "valu_per_wave_sd": float(costs.std()), "valu_per_wave_min": float(costs.min()), "valu_per_wave_max": float(costs.max())}
    return costs, info


def bc1_wave_costs(n, rng):
    """memory round trips of n waves of K-BC1: window + filter (2), one per look-up round, one more for a second-bucket walk, the store (0.5)"""
    valid = rng.binomial(64, 0.5, n)
    pairs = valid + rng.binomial(4 * valid, 0.55)        # mean ~ 102 per wave (smi_bc.hip: "~ 102 pairs per wave on the bench's reads = two rounds")
    rounds = (pairs + 63) // 64
    walk = rng.random(n) < 1.0 / 9.0
    costs = 2.5 + rounds + walk
    return costs, {"pairs_per_wave_mean": float(pairs.mean()), "rounds_mean": float(rounds.mean()),
                   "share_of_waves_by_rounds": {str(r): float((rounds == r).mean()) for r in range(int(rounds.max()) + 1)},
                   "share_of_waves_with_a_second_bucket": float(walk.mean()), "trips_per_wave_mean": float(costs.mean()), "trips_per_wave_sd": float(costs.std())}


def _policies(costs, n_slots, grid_blocks):
    out = {"a_blocks": simulate(costs, n_slots, "blocks", 4, grid_blocks), "b_waves": simulate(costs, n_slots, "waves"),
           "c_claim": simulate(costs, n_slots, "claim")}
    base = out["a_blocks"]["makespan"]
    for v in out.values():
        v["makespan_vs_blocks"] = v["makespan"] / base
    return out


def main():
    sample = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    rng = np.random.default_rng(36)
    n_reads = 10_000_000
    sc, sc_info = scan_wave_costs(sample, rng)
    scan_units = 2 * n_reads // 64
    scan_costs = sc[rng.integers(0, sample, scan_units)]             # the launch's 312,500 waves: the sample's waves drawn with replacement
    bc_units = (n_reads + 63) // 64
    bc_costs, bc_info = bc1_wave_costs(bc_units, rng)
    out = {
        "what": "wave scheduling of K-SCAN and K-BC1 on 1,024 SIMDs, CPU model (tools/sched_model.py): idle wave-slot time and tail of (a) blocks of "
                "four waves freed together, (b) one-wave units handed out by hardware, (c) resident waves that claim units from a counter",
        "k_scan": {"slots": N_SIMD * 4, "units": scan_units, "unit": "VALU instructions of a wave (a slot's time at a quarter of a SIMD's issue rate)",
                   "work": sc_info, "policies": _policies(scan_costs, N_SIMD * 4, 256 * 64)},
        "k_bc1": {"slots": N_SIMD * 8, "units": bc_units, "unit": "dependent memory round trips of a wave", "work": bc_info,
                  "policies": _policies(bc_costs, N_SIMD * 8, None)},
        "leaves_out": [
            "memory latency and its variation: a K-SCAN wave's time is its instruction count, a K-BC1 wave's its count of dependent round trips",
            "the dispatcher's own rate and the start of a block or wave (kernel arguments, LDS allocation): (b) and (c) differ only in the order in "
            "which the units are taken (in order / from sixteen ranges)",
            "issue sharing: a SIMD with an empty slot is taken to issue no faster for the waves it still holds, which makes every idle slot a full loss "
            "(an upper bound on what (a) costs an issue-bound kernel)",
            "the atomic of a claim and the fill that sets the counter",
            "K-BC1's pairs are drawn to the kernel's mean, not derived from the bench's reads",
        ],
    }
    for k in ("k_scan", "k_bc1"):
        p = out[k]["policies"]
        out[k]["predicted_gain_of_claim_over_blocks"] = 1.0 - p["c_claim"]["makespan"] / p["a_blocks"]["makespan"]
    print(json.dumps({k: {"gain": out[k]["predicted_gain_of_claim_over_blocks"],
                          "idle_share": {n: p["idle_share_of_slot_time"] for n, p in out[k]["policies"].items()}} for k in ("k_scan", "k_bc1")}))
    if len(sys.argv) > 2:
        json.dump(out, open(sys.argv[2], "w"), indent=1)


if __name__ == "__main__":
    main()
