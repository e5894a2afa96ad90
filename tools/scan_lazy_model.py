#!/usr/bin/env python3
"""How often K-SCAN's lazily computed statistics are asked for, on the bench generator's reads (CPU: the gate model of scan_gate_model.py and the
oracle's alignment statistics, folded as the kernel folds them):
  - TSO: ends whose winner is present (accepted with round(ne) <= 5) and not passed (nmis > 5) -- phase C counts the runs of a wave's winners when
    one of its 64 ends is such an end
  - adapter (3', the 10-mer): ends on which an acceptable candidate ties with an acceptable incumbent on the best ne -- the fold computes end5 keys
    then, and a wave executes that branch when one of its lanes does
No GPU needed.  usage: scan_lazy_model.py [waves] [out.json]"""
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
AD10 = "CTTCCGATCT"
LETTER = {1: "A", 2: "G", 4: "C", 8: "T", 15: "N"}


def main():
    waves = int(sys.argv[1]) if len(sys.argv) > 1 else 625
    synth = importlib.import_module(graft.load_package().__name__ + ".synth")
    sor = graft.load_oracle()
    sor.build()
    L = sor.lib()
    L.sor_nw_stats.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    o9, f2 = np.zeros(9, dtype=np.int32), np.zeros(2, dtype=np.float32)

    def stats(pattern, sl):
        assert L.sor_nw_stats(pattern, sl, o9.ctypes.data, f2.ctypes.data, None) == 0
        return float(f2[0]), int(o9[2]), bool(o9[1])     # ne, nmis, six terminal matches

    wl = synth.make_whitelist(200_000, seed=1, device="cpu")
    used = synth.pick_used(wl, 5000, seed=2)
    rd = synth.gen_reads(32 * waves, used, seed=1000, device="cpu")   # the timed step's generator call (bench.py: seed 1000 + chunk)
    ends = gm.scan_ends(rd)
    n_ends = ends.shape[0]
    text = ["".join(LETTER[int(c)] for c in e).encode() for e in ends]
    tm = gm.gate_masks(ends, gm.TSO, gm.TSO_WINDOW)
    am = gm.gate_masks(ends, AD10, ends.shape[1])
    need = np.zeros(n_ends, dtype=bool)
    present = np.zeros(n_ends, dtype=bool)
    tie = np.zeros(n_ends, dtype=bool)
    has_t = np.zeros(n_ends, dtype=bool)
    n_tso = n_ad = 0
    tso, ad = gm.TSO.encode(), AD10.encode()
    for e in range(n_ends):
        # the TSO fold: first best accepted position; a candidate with ne > 5 makes the scan jump (AdapterTSOanalyzer L96-106)
        best, skip, w_nmis = math.inf, 0, None
        for p in (np.nonzero(tm[e])[0] + 1).tolist():
            if p < skip:
                continue
            ne, nmis, _ = stats(tso, text[e][p - 1:p + 15])
            n_tso += 1
            if math.floor(np.float32(ne) + np.float32(0.5)) <= 5 and ne < best:
                best, w_nmis = ne, nmis
            if ne > 5.0:
                skip = p + max(1, math.floor(np.float32(ne - 5.0) + np.float32(0.5)) - 1)
        present[e] = w_nmis is not None
        need[e] = present[e] and w_nmis > 5
        # the adapter fold of an end with a polyT: positions 1 .. pe - 12
        bt = sor.find_polyt(np.where(ends[e] == 15, 15, ends[e]).astype(np.uint8))
        if bt is None:
            continue
        has_t[e] = True
        a_best, a_have = math.inf, False
        for p in (np.nonzero(am[e][:max(bt[1] - 12, 0)])[0] + 1).tolist():
            ne, nmis, term6 = stats(ad, text[e][p - 1:p + 9])
            n_ad += 1
            if ne < a_best:
                a_best, a_have = ne, False
            if ne == a_best and (nmis <= 3 or term6):
                if a_have:
                    tie[e] = True
                a_have = True
    per_read = need.reshape(-1, 2).any(1)
    out = {
        "what": "how often K-SCAN's lazy branches are entered on the bench generator's reads (CPU model, tools/scan_lazy_model.py)",
        "reads": n_ends // 2, "waves": waves,
        "tso_candidates_aligned_per_end": n_tso / n_ends, "adapter_candidates_aligned_per_end_with_polyT": n_ad / max(int(has_t.sum()), 1),
        "share_of_ends_with_a_tso_winner": float(present.mean()),
        "share_of_reads_with_an_end_present_not_passed": float(per_read.mean()),
        "share_of_ends_present_not_passed": float(need.mean()),
        "share_of_waves_entering_the_rescue_branch": float(need.reshape(waves, 64).any(1).mean()),
        "share_of_ends_with_polyT": float(has_t.mean()),
        "share_of_ends_with_a_tie_on_best_ne": float(tie.mean()),
        "share_of_polyT_ends_with_a_tie_on_best_ne": float(tie[has_t].mean()) if has_t.any() else 0.0,
        "share_of_waves_entering_the_tie_branch": float(tie.reshape(waves, 64).any(1).mean()),
    }
    print(json.dumps(out))
    if len(sys.argv) > 2:
        json.dump(out, open(sys.argv[2], "w"), indent=1)


if __name__ == "__main__":
    main()
