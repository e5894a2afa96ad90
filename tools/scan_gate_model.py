#!/usr/bin/env python3
"""CPU model of K-SCAN's TSO 4-mer gate and of its isolated-candidate rule on the bench generator's reads: how many gated TSO positions a
wave of 64 read ends has, how many of them are isolated (no other candidate of the end among the next 26 positions), and in what share of
the waves the pre-filter of the isolated candidates can save an alignment round at all, i.e.
    ceil(total / 64) > ceil((total - isolated) / 64)
(the filter drops isolated candidates only, so the right-hand side is the fewest rounds it can leave).  No GPU needed.
usage: scan_gate_model.py [waves] [out.json]"""
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

TSO = "AACGCAGAGTACATGG"
CODE = {"A": 1, "G": 2, "C": 4, "T": 8}
TSO_WINDOW = 90
JUMP = 26


def gate_masks(ends4, pattern, n_pos):
    """ends4: [n_ends, 208] 4-bit codes in scan orientation -> bool [n_ends, n_pos]: >= 2 of the pattern's 4-mers match on the diagonal
    (Kmers.nKmersMatching_4mer > 1 as gate64 computes it: bases past the end match nothing)"""
    n, E = ends4.shape
    L = len(pattern)
    pad = np.zeros((n, E + L + n_pos), dtype=np.int64)
    pad[:, :E] = ends4
    match = np.stack([(pad[:, i:i + n_pos] & CODE[pattern[i]]) != 0 for i in range(L)])  # [L, n, n_pos]: read base p + i matches pattern base i
    kmers = np.zeros((n, n_pos), dtype=np.int64)
    for i in range(L - 3):
        kmers += (match[i] & match[i + 1] & match[i + 2] & match[i + 3])
    return kmers >= 2


def isolated(mask):
    """candidates without another candidate of their end among the next JUMP positions"""
    n, P = mask.shape
    later = np.zeros_like(mask)
    for d in range(1, JUMP + 1):
        later[:, :P - d] |= mask[:, d:]
    return mask & ~later


def isolated_words(mask):
    """`isolated` as the shipped kernels compute it for the TSO window of 90 positions: the candidate bits on three 32-bit words, s = the mask one
    position down, then three steps that OR two shifted copies into s (distances 1 -> 1..3 -> 1..9 -> 1..26)"""
    n, P = mask.shape
    assert P == TSO_WINDOW
    m32 = (1 << 32) - 1
    out = np.zeros_like(mask)

    def align(hi, lo, s):
        return (((hi << 32) | lo) >> s) & m32

    for i in range(n):
        m = 0
        for p in np.nonzero(mask[i])[0].tolist():
            m |= 1 << p
        t = [(m >> (32 * k)) & m32 for k in range(3)]
        s = [align(t[1], t[0], 1), align(t[2], t[1], 1), t[2] >> 1]
        for k1, k2 in ((1, 2), (3, 6), (9, 17)):
            s = [s[0] | align(s[1], s[0], k1) | align(s[1], s[0], k2), s[1] | align(s[2], s[1], k1) | align(s[2], s[1], k2), s[2] | (s[2] >> k1) | (s[2] >> k2)]
        iso = m & ~(s[0] | (s[1] << 32) | (s[2] << 64))
        for p in range(P):
            out[i, p] = bool((iso >> p) & 1)
    return out


def scan_ends(rd):
    """both ends of every read in scan orientation as 4-bit codes: [2 n, 208], end 2 i = head, 2 i + 1 = reverse complement of the tail"""
    lut = np.array([1, 2, 4, 8, 15], dtype=np.int64)
    head, tail = rd["head"].numpy().astype(np.int64), rd["tail"].numpy().astype(np.int64)
    t = tail[:, ::-1]
    t = np.where(t > 3, t, 3 - t)
    ends = np.empty((2 * head.shape[0], head.shape[1]), dtype=np.int64)
    ends[0::2], ends[1::2] = lut[head], lut[t]
    return ends


def main():
    waves = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    synth = importlib.import_module(graft.load_package().__name__ + ".synth")
    wl = synth.make_whitelist(200_000, seed=1, device="cpu")
    used = synth.pick_used(wl, 5000, seed=2)
    rd = synth.gen_reads(32 * waves, used, seed=1000, device="cpu")  # the timed step's generator call (bench.py: seed 1000 + chunk)
    tm = gate_masks(scan_ends(rd), TSO, TSO_WINDOW)
    iso = isolated(tm)
    total = tm.reshape(waves, 64, -1).sum((1, 2))
    n_iso = iso.reshape(waves, 64, -1).sum((1, 2))
    rounds = lambda x: (x + 63) // 64  # noqa: E731
    can_save = rounds(total) > rounds(total - n_iso)
    out = {
        "what": "TSO gate candidates per wave of 64 read ends on the bench generator's reads (CPU model, tools/scan_gate_model.py)",
        "waves": waves,
        "gated_per_wave": {"mean": float(total.mean()), "sd": float(total.std()), "min": int(total.min()), "max": int(total.max())},
        "isolated_per_wave": {"mean": float(n_iso.mean()), "sd": float(n_iso.std())},
        "share_of_waves_total_le_64": float((total <= 64).mean()),
        "share_of_waves_filter_cannot_save_a_round": float((~can_save).mean()),
    }
    print(json.dumps(out))
    if len(sys.argv) > 2:
        json.dump(out, open(sys.argv[2], "w"), indent=1)


if __name__ == "__main__":
    main()
