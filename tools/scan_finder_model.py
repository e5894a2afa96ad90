#!/usr/bin/env python3
"""CPU model of the tail of K-SCAN's bit-parallel polyT finder (smi_scan.hip find_polyt_bits, the code behind `first`): the extension of `start`
by the strides 20, 15, 10, 5, 4, 3, 2, 1, the walk back to the last position that passes `back`, and the three forward steps -- once as the loops
of PolyATSearcher.java:L223-230 / L122-172 (tail_loops: what the finder ran until NOTES R6.28 and what -DSMI_SCAN_FINDER_TAIL_LOOPS=1 still
compiles) and once as the mask operations of the kernel (tail_masks), both over Python integers as bit masks:
    T   exact-T bits of an end (bit p = base p is a T, not an N)
    G   the extension's probe mask: bit p = p < window and >= 10 T's in [p + 1, p + 16)
tests/test_scan_finder_cpu.py compares the two on random and on structured masks.  Run as a program, it reports on the bench generator's reads
(the timed step's generator call) the loops' trip counts -- per end, and per wave of 64 ends as the maximum over its lanes, which is what a wave
executes -- and how often the mask code takes each of its slow paths, per end and per wave.  No GPU needed.
usage: scan_finder_model.py [waves] [out.json]"""
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_gate_model as gm  # noqa: E402

ML = 15
INC = (20, 15, 10, 5, 4, 3, 2, 1)
M64 = (1 << 64) - 1
STRIDE_MASK = {s: sum(1 << b for b in range(s, 64, s)) for s in INC}
FOUR20 = 1 | 1 << 20 | 1 << 40 | 1 << 60
BACK_BELOW = 40          # kFinderBackBelow: positions of the window below endpos = start + 14


def popc(x):
    return bin(x).count("1")


def ctz(x):
    return (x & -x).bit_length() - 1


def masks_of(codes, window=150):
    """4-bit codes of an end -> (T, G, first): first = the lowest entry position below `window`, or -1 (the finder's branch-free front)"""
    T = 0
    for p, c in enumerate(codes):
        if int(c) == 8:
            T |= 1 << p
    G, first = 0, -1
    for p in range(window):
        k = popc((T >> (p + 1)) & 0x7FFF)
        if k >= 10:
            G |= 1 << p
        if first < 0 and k >= 12 and (T >> p) & 1 and popc((T >> p) & 31) >= 3:
            first = p
    return T, G, first


M32 = (1 << 32) - 1
SUM3, MAJ3, AND3, ORAND3, ANDOR3 = 0x96, 0xE8, 0x80, 0xF8, 0xE0   # smi_scan.hip kSum3 .. kAndOr3


def bit3(imm, a, b, c):
    """v_bitop3_b32 on 32-bit words: bit (a << 2 | b << 1 | c) of the immediate, position by position"""
    r = 0
    for idx in range(8):
        if (imm >> idx) & 1:
            r |= (a if idx & 4 else ~a) & (b if idx & 2 else ~b) & (c if idx & 1 else ~c)
    return r & M32


def alignbit(hi, lo, s):
    return (((hi << 32) | lo) >> s) & M32


def front_words(T, window=150):
    """the finder's branch-free front operation for operation (find_polyt_bits up to `first`: the bit-sliced five-counts and fifteen-counts on 32-bit
    words in their three-input forms, the entry mask, the probe mask) -> (G, first); masks_of says the same with a loop over the positions"""
    tw = [(T >> (32 * k)) & M32 for k in range(6)]
    c5 = [[0] * 6 for _ in range(3)]
    for k in range(6):
        up = tw[k + 1] if k + 1 < 6 else 0
        s1, s2, s3, s4 = (alignbit(up, tw[k], s) for s in (1, 2, 3, 4))
        x, k1 = bit3(SUM3, tw[k], s1, s2), bit3(MAJ3, tw[k], s1, s2)
        c5[0][k], k2 = bit3(SUM3, x, s3, s4), bit3(MAJ3, x, s3, s4)
        c5[1][k], c5[2][k] = k1 ^ k2, k1 & k2
    ge12, ge10 = [0] * 6, [0] * 6
    for k in range(5):
        b = [alignbit(c5[j][k + 1], c5[j][k], 5) for j in range(3)]
        c = [alignbit(c5[j][k + 1], c5[j][k], 10) for j in range(3)]
        k0 = bit3(MAJ3, c5[0][k], b[0], c[0])
        t1, k1a = bit3(SUM3, c5[1][k], b[1], c[1]), bit3(MAJ3, c5[1][k], b[1], c[1])
        r1, k1b = t1 ^ k0, t1 & k0
        t2, k2a = bit3(SUM3, c5[2][k], b[2], c[2]), bit3(MAJ3, c5[2][k], b[2], c[2])
        r2, k2b = bit3(SUM3, t2, k1a, k1b), bit3(MAJ3, t2, k1a, k1b)
        r3 = k2a | k2b
        ge12[k], ge10[k] = r3 & r2, bit3(ANDOR3, r3, r2, r1)
    top = popc(tw[5] & 0x7FFF)
    ge12[5], ge10[5] = int(top >= 12), int(top >= 10)
    G, first = 0, -1
    for k in range(4, -1, -1):
        keep = window - 32 * k
        below = M32 if keep >= 32 else (0 if keep <= 0 else (1 << keep) - 1)
        entry = bit3(AND3, alignbit(ge12[k + 1], ge12[k], 1), tw[k], bit3(ORAND3, c5[2][k], c5[1][k], c5[0][k])) & below
        G |= (alignbit(ge10[k + 1], ge10[k], 1) & below) << (32 * k)
        if entry:
            first = 32 * k + ctz(entry)
    return G, first


def back_mask_words(w):
    """the walk back's mask over a 64-bit window of exact-T bits as the kernel computes it: two three-input operations per 32-bit half"""
    w &= M64
    l1, l2, l3, l4 = ((w << s) & M64 for s in (1, 2, 3, 4))
    out = 0
    for h in (0, 32):
        half = lambda x: (x >> h) & M32   # noqa: E731
        out |= bit3(AND3, half(w), half(l1), bit3(MAJ3, half(l2), half(l3), half(l4))) << h
    return out


def back_ok(T, e):
    """lambda$findpolyAT$3 L122-142 at position e: T at e, >= 2 T in the last 2, >= 3 in the last 4, >= 4 in the last 5"""
    x = (T >> (e - 4)) & 31
    return bool((x >> 4) & 1 and popc((x >> 3) & 3) >= 2 and popc((x >> 1) & 15) >= 3 and popc(x) >= 4)


def forward(T, endpos, window, look):
    """the three forward steps (L145-147, L156-158, L171-172); look(p) -> exact-T bits from p on"""
    n = window + ML + 10
    while n > endpos + 6 and popc(look(endpos + 1) & 31) > 3:
        endpos += 5
    while n > endpos + 4 and popc(look(endpos + 1) & 7) > 1:
        endpos += 3
    while endpos < n - 1 and look(endpos + 1) & 1:
        endpos += 1
    return endpos


def tail_loops(T, G, first, window=150, stats=None):
    """-> (start, endpos behind the walk back, end1); stats: dict that receives the trip counts"""
    start = first
    goes = []
    for s in INC:
        n_go = 1
        while (G >> (start + s)) & 1:
            start += s
            n_go += 1
        goes.append(n_go)
    endpos = start + ML - 1
    e = endpos
    while e > 4 and not back_ok(T, e):
        e -= 1
    n_fwd = [0]

    def look(p):
        n_fwd[0] += 1
        return T >> p

    end = forward(T, e, window, look)
    if stats is not None:
        stats.update(go=goes, advance=start - first, back=endpos - e, fwd=n_fwd[0])
    return start, e, end + 1


def tail_masks(T, G, first, window=150, stats=None):
    """the kernel's tail, operation for operation on 64-bit registers; stats receives the slow paths taken"""
    slow = {"ext": 0, "back": 0, "fwd": 0}
    start = first
    nw = ~(G >> (first + 20)) & M64          # stride 20: a register of its own, taken at first + 20: four probes
    z = nw & FOUR20
    while z == 0:
        slow["ext"] += 1
        start += 80
        nw = ~(G >> (start + 20)) & M64
        z = nw & FOUR20
    start += ctz(z)
    gbase = start
    nw = ~(G >> start) & M64
    for s in INC[1:]:
        ms = STRIDE_MASK[s]
        z = nw & ms
        while z == 0:
            slow["ext"] += 1
            if gbase == start:
                start += s * (63 // s)
            gbase = start
            nw = ~(G >> start) & M64
            z = nw & ms
        adv = ctz(z) - s
        start += adv
        nw >>= adv
    endpos = start + ML - 1
    win = [max(endpos - BACK_BELOW, 0)]
    bits = [(T >> win[0]) & M64]
    w = bits[0]
    l1, l2, l3, l4 = (w << 1) & M64, (w << 2) & M64, (w << 3) & M64, (w << 4) & M64
    back = w & l1 & ((l2 & l3) | (l4 & (l2 ^ l3)))
    back &= ((2 << (endpos - win[0])) - 1) & (M64 ^ (15 if win[0] else 31))
    if back:
        e = win[0] + back.bit_length() - 1
    else:
        e = win[0] + 3 if win[0] else 4
        if e > 4:
            slow["back"] += 1
        while e > 4 and not back_ok(T, e):
            e -= 1

    def look(p):
        if p < win[0] or p + 5 > win[0] + 64:
            slow["fwd"] += 1
            win[0], bits[0] = p, (T >> p) & M64
        return bits[0] >> (p - win[0])

    end = forward(T, e, window, look)
    if stats is not None:
        stats.update(slow)
    return start, e, end + 1


def main():
    waves = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    synth = importlib.import_module(gm.graft.load_package().__name__ + ".synth")
    wl = synth.make_whitelist(200_000, seed=1, device="cpu")
    used = synth.pick_used(wl, 5000, seed=2)
    rd = synth.gen_reads(32 * waves, used, seed=1000, device="cpu")   # the timed step's generator call (bench.py: seed 1000 + chunk)
    ends = gm.scan_ends(rd)
    n_ends = ends.shape[0]
    has = np.zeros(n_ends, dtype=bool)
    go = np.zeros((n_ends, 8), dtype=np.int64)
    adv = np.zeros(n_ends, dtype=np.int64)
    back = np.zeros(n_ends, dtype=np.int64)
    fwd = np.zeros(n_ends, dtype=np.int64)
    slow = np.zeros((n_ends, 3), dtype=np.int64)
    first_window_exhausted = np.zeros(n_ends, dtype=bool)
    for i in range(n_ends):
        T, G, first = masks_of(ends[i])
        if first < 0:
            continue
        has[i] = True
        a, b = {}, {}
        r_loop, r_mask = tail_loops(T, G, first, stats=a), tail_masks(T, G, first, stats=b)
        assert r_loop == r_mask, (i, r_loop, r_mask)
        go[i], adv[i], back[i], fwd[i] = a["go"], a["advance"], a["back"], a["fwd"]
        slow[i] = b["ext"], b["back"], b["fwd"]
        first_window_exhausted[i] = a["advance"] >= 44
    per_read = has.reshape(-1, 2)
    w = lambda x: x.reshape(waves, 64, *x.shape[1:])   # noqa: E731
    go_wave = w(go).max(1)   # a loop runs as often as the wave's worst lane asks
    out = {
        "what": "the tail of K-SCAN's bit-parallel polyT finder on the bench generator's reads (CPU model, tools/scan_finder_model.py)",
        "reads": n_ends // 2, "waves": waves,
        "share_of_ends_with_polyT": float(has.mean()),
        "reads_with_polyT_on_both_ends": int(per_read.all(1).sum()),
        "loops": {
            "strides": list(INC),
            "go_evaluations_per_wave": float(go_wave.sum(1).mean()),
            "go_evaluations_per_wave_by_stride": [float(x) for x in go_wave.mean(0)],
            "go_evaluations_per_end_with_polyT": float(go[has].sum(1).mean()),
            "advance_of_start": {"mean": float(adv[has].mean()), "max": int(adv[has].max()),
                                 "share_of_polyT_ends_ge_44": float(first_window_exhausted[has].mean())},
            "walk_back": {"mean": float(back[has].mean()), "max": int(back[has].max())},
            "forward_evaluations_per_wave": float(w(fwd).max(1).mean()),
            "forward_evaluations_per_end_with_polyT": float(fwd[has].mean()),
        },
        "masks_slow_paths": {
            name: {"per_end_with_polyT": float((slow[has, j] > 0).mean()), "per_wave": float((w(slow[:, j]) > 0).any(1).mean()),
                   "refills_per_wave_worst_lane": float(w(slow[:, j]).max(1).mean())}
            for j, name in enumerate(("extension_window_exhausted", "walk_back_not_decided_by_window", "forward_steps_leave_window"))
        },
        "same_result_on_every_end": True,
    }
    print(json.dumps(out))
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        json.dump(out, open(sys.argv[2], "w"), indent=1)


if __name__ == "__main__":
    main()
