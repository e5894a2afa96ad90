#!/usr/bin/env python3
"""How often a rescue rule of scanReadForTSOs really reads the runs of a TSO winner, on the bench generator's reads (CPU: the gate model of
scan_gate_model.py and the oracle's alignment statistics, folded as the kernel folds them -- the method of scan_lazy_model.py with the partner end's
verdict added).  The rules apply when NEITHER end of a read is found (found = present and passed by nmis) and read the runs of the ends that are
present, so a winner's runs are read only on
  an end that is present (accepted with round(ne) <= 5) and not passed (nmis > 5) whose partner end is not found
K-SCAN's shipped kernels keep no path of a TSO candidate (smi_nw.h nw_counts) and align such an end's winner again in phase C, behind one ballot: a
wave pays for that when one of its 64 ends is such an end.
No GPU needed.  usage: scan_rescue_model.py [waves] [out.json]"""
import ctypes
import importlib
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_gate_model as gm  # noqa: E402

graft = gm.graft
LETTER = {1: "A", 2: "G", 4: "C", 8: "T", 15: "N"}


def main():
    waves = int(sys.argv[1]) if len(sys.argv) > 1 else 625
    synth = importlib.import_module(graft.load_package().__name__ + ".synth")
    sor = graft.load_oracle()
    sor.build()
    L = sor.lib()
    L.sor_nw_stats.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    o9, f2 = np.zeros(9, dtype=np.int32), np.zeros(2, dtype=np.float32)

    def stats(sl):
        assert L.sor_nw_stats(tso, sl, o9.ctypes.data, f2.ctypes.data, None) == 0
        return float(f2[0]), int(o9[2])     # ne, nmis

    wl = synth.make_whitelist(200_000, seed=1, device="cpu")
    used = synth.pick_used(wl, 5000, seed=2)
    rd = synth.gen_reads(32 * waves, used, seed=1000, device="cpu")   # the timed step's generator call (bench.py: seed 1000 + chunk)
    ends = gm.scan_ends(rd)
    n_ends = ends.shape[0]
    text = ["".join(LETTER[int(c)] for c in e).encode() for e in ends]
    tm = gm.gate_masks(ends, gm.TSO, gm.TSO_WINDOW)
    tso = gm.TSO.encode()
    present = np.zeros(n_ends, dtype=bool)
    passed = np.zeros(n_ends, dtype=bool)
    n_aligned = 0
    for e in range(n_ends):
        # the TSO fold: first best accepted position; a candidate with ne > 5 makes the scan jump (AdapterTSOanalyzer L96-106)
        best, skip, w_nmis = math.inf, 0, None
        for p in (np.nonzero(tm[e])[0] + 1).tolist():
            if p < skip:
                continue
            ne, nmis = stats(text[e][p - 1:p + 15])
            n_aligned += 1
            if math.floor(np.float32(ne) + np.float32(0.5)) <= 5 and ne < best:
                best, w_nmis = ne, nmis
            if ne > 5.0:
                skip = p + max(1, math.floor(np.float32(ne - 5.0) + np.float32(0.5)) - 1)
        present[e] = w_nmis is not None
        passed[e] = present[e] and w_nmis <= 5
    found = present & passed
    partner_found = found.reshape(-1, 2)[:, ::-1].reshape(-1)
    not_passed = present & ~passed
    need = not_passed & ~partner_found
    out = {
        "what": "how often a rescue rule reads a TSO winner's runs on the bench generator's reads (CPU model, tools/scan_rescue_model.py)",
        "reads": n_ends // 2, "waves": waves,
        "tso_candidates_gated_per_wave": float(tm.sum()) / waves,
        "tso_candidates_aligned_by_the_fold_per_wave": n_aligned / waves,
        "share_of_ends_with_a_tso_winner": float(present.mean()),
        "ends_present_not_passed": int(not_passed.sum()),
        "share_of_ends_present_not_passed": float(not_passed.mean()),
        "share_of_waves_with_an_end_present_not_passed": float(not_passed.reshape(waves, 64).any(1).mean()),
        "ends_present_not_passed_partner_not_found": int(need.sum()),
        "share_of_ends_present_not_passed_partner_not_found": float(need.mean()),
        "waves_with_such_an_end": int(need.reshape(waves, 64).any(1).sum()),
        "share_of_waves_with_such_an_end": float(need.reshape(waves, 64).any(1).mean()),
        "such_ends_per_wave_that_has_one": float(need.sum()) / max(int(need.reshape(waves, 64).any(1).sum()), 1),
    }
    print(json.dumps(out))
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        json.dump(out, open(sys.argv[2], "w"), indent=1)


if __name__ == "__main__":
    main()
