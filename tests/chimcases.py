"""Hand-built reads for the chimera splitter (K-CHIM): every case sits ON one edge of the kernels or of the reference's rules, and its twin
one base past it.  No GPU, no product import; deterministic.  tests/test_chim_cases_cpu.py proves with pymodel_chimera that every case means what
its `intent` says; tests/test_chim_edges_gpu.py runs the batches through the kernels.

Coordinates.  A pattern whose first base is read[i] has scan position i + 1 (1-based).  `begin` of a match is the 1-based coordinate of the
pattern's own 5' end: i + 1 for a forward TSO / forward adapter, the last base of the reverse complement for the reverse ones.  A polyT stretch
whose first T is read[t] triggers aTscan at pos = t (begin t + 1).  aTscan's window is, by the reference's arithmetic, the 14 bases read[pos + 1 ..
pos + 14] plus the base read[off + 13] once more for EVERY position of the read (`extra`): builders keep read[233] a C unless the case is about it.

Plane phase.  Read r starts at plane word (offsets[r] >> 5) + 5 r (plane_start, kReadPadWords = 5); k_chima_flat takes tiles of 256 words.

Families built: S1 - S5, T1 (TSO and adapter rule), T2 - T10, K1 (d = 30 .. 33), K2, K3, C1 - C5, and of C6 the stretch queue, the
adapter-alignment queue and one region of the position queue.  Not built, with the argument:
  * T8 is built at the level of its rule: two equal-best offsets 1 apart (the second removed) and 2 apart (both kept), the match taken from the first.
    Not built: a first best offset that passes the score and fails `nmis <= ad_max`, which is the only way the second of two kept offsets could
    become the match (round(x - 0.9 lead) <= ad_max < x - trailing read gaps, with the same float score at the second offset); T7 therefore holds
    the nmis rule only through nErrors = ad_max against ad_max + 1.
  * K1 d = 1: a position one base in front of an exact TSO shares no two 4-mers with it on the diagonal (the shipped patterns have no self-overlap at
    shift 1), so it is never gated and cannot be "gated and over the bound".
  * A closure of 31 against 32 cannot show in a RESULT.  Proof: a gated position g has nErrors <= #x <= 31 (27-base pattern; the bound in the comment
    above kDmax in smi_chimera.hip), so its skip is delta = round(nErrors - max) - 1 <= round(31 - 5) - 1 = 25 <= 30.  Let n be the first NEEDED
    position behind g, at n - g = 31 exactly.  Every gated position in (g, n) is less than 31 in front of n, so it is needed under either closure and its
    alignment is folded in either way; g itself only decides which positions of (g, g + delta) are visited, and g + delta <= g + 30 < n.  Whether the
    fold knows delta(g) or takes it as 1, the positions of (g, n) that differ are not gated ... or are needed and then g is needed through them
    (they are < 31 behind g).  So the accepted set is the same.  K1 / K2 hold the kernels to the reference AROUND 31 / 32; the count of queued
    positions (Context.chimera_last_counts()["positions"] under SMI_CHIM_A1) is what tells 31 from 32, and test_chim_edges_gpu.py asserts it on K1.
  * C4 (512 gated positions) is a cap of the SMI_CHIM_A1 select kernel only; the default select kernel has none.  C5 has no counter: the result is checked.
  * C6 position queue: the whole queue holds max(48 n_list, 65536) positions, which needs > 2 M bases of dense TSO fragments to pass.  One of its 64
    regions holds 1,024 positions for the sixteen reads of a workgroup of k_chimb_select2; `C6_posq` passes that, which is the same branch.
  * No case declares rc != 0: the oracle reports it only for a cut behind the read's end or in front of the previous cut.  The 100-base rule removes
    every cut less than 100 behind its predecessor (negative distances included), and a REV_ADAPTER cut is begin + 25 with begin <= at.end + bc_umi + 40
    and at.end <= len - 236, so neither can happen for a sequence; CHIM_RANGE is still asserted to be absent on every read.
"""
import random

import pymodel_chimera as pm
from pymodel_scan import count_errors, enc, kmers_matching, needleman

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
CFG = {
    False: dict(five_prime=False, tso="AAGCAGTGGTATCAACGCAGAGTACAT", ad="CTACACGACGCTCTTCCGATCT", tso_max=6, ad_max=5, bc_umi=28),
    True: dict(five_prime=True, tso="CTACACGACGCTCTTCCGATCT", ad="AAGCAGTGGTATCAACGCAGAGTAC", tso_max=5, ad_max=5, bc_umi=0),
}
OFF = 220          # aTscan: window 150 + 70
TILE = 256
MODEL_MAX = 3000   # longer reads are compared with the oracle alone


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def model(read, five_prime):
    c = CFG[bool(five_prime)]
    return pm.find_split_positions(read, c["tso"], c["ad"], c["tso_max"], c["ad_max"], c["bc_umi"])


_FILLERS = {}


def filler(rng, n, five_prime=None):
    """random ACGT with no match at all in the model (either configuration unless one is named); read[233] is a C"""
    while True:
        s = rnd(rng, n)
        if n > OFF + 13:
            s = s[:OFF + 13] + "C" + s[OFF + 14:]
        if n < 240 or all(not model(s, fp)[2] for fp in ((False, True) if five_prime is None else (five_prime,))):
            return s


def pooled_filler(n):
    """a filler of n bases, the same every time (the fillers in front of a target only set its plane phase)"""
    if n not in _FILLERS:
        _FILLERS[n] = filler(random.Random(9000 + n), n)
    return _FILLERS[n]


def offsets_of(reads):
    o = [0]
    for r in reads:
        o.append(o[-1] + len(r))
    return o


def plane_word(offsets, r, q):
    """plane word of base q of read r: a copy of plane_start (smi_internal.h)"""
    return (offsets[r] >> 5) + 5 * r + (q >> 5)


def planes_words(total, n):
    """a copy of smi_read_planes_words"""
    return 4 * ((total >> 5) + 5 * (n + 1) + 8)


def shift_to(batch, target, q, word_in_tile, bit, rng=None):
    """fillers in front of the batch, and random bases in front of the target, until base q of the target lies at word `word_in_tile` of its tile, bit `bit`
    -> (batch, target, q)"""
    rng = rng or random.Random(77)
    batch = list(batch)
    pad = (bit - q) % 32
    if pad:
        batch[target] = rnd(rng, pad) + batch[target]
        q += pad
    while True:
        d = (word_in_tile - plane_word(offsets_of(batch), target, q)) % TILE
        if d == 0:
            return batch, target, q
        if d < 6:
            k = 20       # too near for one read (a read costs five pad words): go round
        elif d >= 5 + 15 and not any(len(x) == 480 for x in batch):
            k = 15       # one scanned filler in every shifted batch
        else:
            k = min(d - 5, 7)  # at most 224 bases: unscanned
        batch.insert(0, pooled_filler(32 * k))
        target += 1


def place(bg, i, s):
    assert 0 <= i and i + len(s) <= len(bg)
    return bg[:i] + s + bg[i + len(s):]


def mutate(s, k, kind, start=8):
    """k edits of one kind in one block from base `start` on: the 4-mers in front of and behind the block still pass the gate"""
    s = list(s)
    for i in range(start, start + k):
        if kind == "sub":
            s[i] = COMP[s[i]]
        elif kind == "del":
            s[i] = ""
        else:
            s[i] = s[i] + COMP[s[i]]
    return "".join(s)


def tso_with_edits(cfg, k, kind="sub", start=8):
    """the configuration's TSO with k edits of one kind (a further argument to the issue's helper: there are two configurations)"""
    return mutate(cfg["tso"], k, kind, start)


ST_T = "TTGTTTTTGTTTTT"   # the smallest polyT trigger: T T, and 11 T in the 14 bases behind the first -- at its first base and nowhere else
ST_A = "AAGAAAAAGAAAAA"


def polya_site(cfg, rng, nuc="T", run=None, ad=None):
    """-> (sequence, index of the first base of the stretch in it, index of the adapter's `begin` base in it).
    T: adapter + BC/UMI + polyT (a forward adapter); A: polyA + rc(BC/UMI) + rc(adapter) (a reverse adapter).  run None: the minimal trigger."""
    ad = cfg["ad"] if ad is None else ad
    gap = rnd(rng, cfg["bc_umi"], "ACG")
    if nuc == "T":
        st = ST_T if run is None else "T" * run
        return ad + gap + st + "C", len(ad) + len(gap), 0
    st = ST_A if run is None else "A" * run
    s = st + rc(gap) + rc(ad)
    return "C" + s, 1, len(s)


# ----------------------------------------------------------------------------------------------------------------------
CASES = []


def add(name, fp, reads, target, **intent):
    CASES.append(dict(name=("5p_" if fp else "3p_") + name, five_prime=fp, reads=list(reads), target=target, intent=intent))


def elements(cfg, rng):
    """the four site kinds of S1: name -> (sequence, index in it of the base that is placed)"""
    t_seq, t_q, _ = polya_site(cfg, rng, "T")
    a_seq, a_q, _ = polya_site(cfg, rng, "A")
    return {"ftso": (cfg["tso"], 0), "rtso": (rc(cfg["tso"]), 0), "polyT": (t_seq, t_q), "polyA": (a_seq, a_q)}


def site_read(rng, fp, n, i, seq, key=0):
    """a filler of n bases with `seq` placed so that seq[key] is read[i]"""
    return place(pooled_filler(n), i - key, seq)


def build_S(fp):
    cfg = CFG[fp]
    rng = random.Random(100 + fp)
    # S1: the first base of the pattern / of the trigger window at the last word of a tile (bits 0, 5, 31) and at the first (bit 0)
    for kind, (seq, key) in elements(cfg, rng).items():
        for word, bit in ((255, 0), (255, 5), (255, 31), (0, 0)):
            q = 320 + bit
            read = site_read(rng, fp, 760, q, seq, key)
            batch, t, q = shift_to([read, pooled_filler(480)], 0, q, word, bit)
            add(f"S1_{kind}_w{word}_b{bit}", fp, batch, t, phase=(q, word, bit), n_matches=1, family="S")
    # S2: the target begins at tile words 254, 255, 0, 1 behind an unscanned, an empty, a one-base and a just-scanned read; a TSO at scan position 70
    fronts = {"239": pooled_filler(239), "empty": "", "one": "G", "240": pooled_filler(240)}
    for fname, front in fronts.items():
        for word in (254, 255, 0, 1):
            read = site_read(rng, fp, 420, 69, cfg["tso"])
            batch, t, _ = shift_to([front, read], 1, 0, word, 0)
            add(f"S2_{fname}_w{word}", fp, batch, t, phase=(0, word, 0), n_matches=1, front=front, family="S")
    # S3: 17,000 bases over three tiles, a site in each; alone, last (the final tile partly beyond the stride), first
    bg = rnd(rng, 17000)
    bg = bg[:OFF + 13] + "C" + bg[OFF + 14:]
    t_seq, _, _ = polya_site(cfg, rng, "T", run=30)
    long_read = place(place(place(bg, 500, cfg["tso"]), 8500, rc(cfg["tso"])), 16400, t_seq)
    add("S3_alone", fp, [long_read], 0, long_sites=3, family="S")
    add("S3_last", fp, [pooled_filler(480), pooled_filler(224), long_read], 2, long_sites=3, family="S")
    add("S3_first", fp, [long_read, pooled_filler(480), pooled_filler(224)], 0, long_sites=3, family="S")
    # S4: the scan bounds
    n, L = 700, len(cfg["tso"])
    for orient, pat in (("f", cfg["tso"]), ("r", rc(cfg["tso"]))):
        for label, i, found in (("70", 69, 1), ("69", 68, 0), ("lenm70", n - 70 - 1, 1), ("lenm69", n - 69 - 1, 0)):
            if orient == "r" and label in ("70", "69"):
                continue
            add(f"S4_tso_{orient}_{label}", fp, [site_read(rng, fp, n, i, pat)], 0, n_matches=found, tso_at=(orient == "r", i + 1, bool(found)),
                twin={"70": "69", "lenm70": "lenm69"}.get(label) and f"S4_tso_{orient}_" + {"70": "69", "lenm70": "lenm69"}[label], family="S")
    for nuc in "TA":
        seq, key, _ = polya_site(cfg, rng, nuc)
        for label, pos, found in (("first", OFF - 1, 1), ("before", OFF - 2, 0), ("last", n - OFF - 1, 1), ("after", n - OFF, 0)):
            read = site_read(rng, fp, n, pos, seq, key)
            if not (pos - key <= OFF + 13 < pos - key + len(seq)):
                read = read[:OFF + 13] + "C" + read[OFF + 14:]
            add(f"S4_trig_{nuc}_{label}", fp, [read], 0, n_matches=found, trigger=(nuc, pos, bool(found)),
                twin={"first": f"S4_trig_{nuc}_before", "last": f"S4_trig_{nuc}_after"}.get(label), family="S")
    for n_len in (240, 439, 440, 441):
        # 240 .. 440: only the TSO scan has positions (aTscan needs len > 2 off); a site in the middle
        read = site_read(rng, fp, n_len, n_len // 2 - 10, cfg["tso"])
        add(f"S4_len{n_len}", fp, [read], 0, n_matches=1, family="S")
    seq, key, _ = polya_site(cfg, rng, "T")
    add("S4_len441_trig", fp, [site_read(rng, fp, 441, OFF - 1, seq, key)], 0, n_matches=1, trigger=("T", OFF - 1, True), family="S")
    # S5: the base at off + 13 counts twice.  pos = off - 1: read[220 .. 233] holds threshold - 1 = 10 of the base, read[233] among them or not
    for nuc, other in (("T", "G"), ("A", "G")):
        ad_f, gap = cfg["ad"], rnd(rng, cfg["bc_umi"], "ACG" if nuc == "T" else "CGT")
        #            219 220 221 ......................... 233
        with_x = nuc * 2 + other + nuc * 4 + other + nuc * 4 + other + other + nuc      # [220 .. 233]: 10, the last of them at 233
        without = nuc * 2 + other + nuc * 4 + other + nuc * 5 + other + other            # [220 .. 233]: 10, read[233] is not one
        for label, st, found in (("doubled", with_x, 1), ("plain", without, 0)):
            if nuc == "T":
                seq, key = ad_f + gap + st + "C", len(ad_f) + len(gap)
            else:
                seq, key = "C" + st + "C" + rc(gap) + rc(ad_f), 1
            read = site_read(rng, fp, n, OFF - 1, seq, key)
            add(f"S5_{nuc}_{label}", fp, [read], 0, doubled=(nuc, found), twin=f"S5_{nuc}_plain" if found else None, family="S")


def build_T(fp):
    cfg = CFG[fp]
    rng = random.Random(200 + fp)
    tso, L = cfg["tso"], len(cfg["tso"])
    rtso = rc(tso)

    def with_sites(n, sites):
        read = pooled_filler(n)
        for i, s in sites:
            read = place(read, i, s)
        return read

    # T1: begin 120 / 121 apart, both orientations
    for orient, pat in (("f", tso), ("r", rtso)):
        for d in (120, 121):
            add(f"T1_{orient}_{d}", fp, [with_sites(900, [(300, pat), (300 + d, pat)])], 0, n_matches=1 if d == 120 else 2,
                twin=f"T1_{orient}_121" if d == 120 else None, family="T")
    # T1 for the adapters' own > 120 rule (prevT_Position / prevA_Position): two polyT sites, two polyA sites, adapter begins 120 / 121 apart
    for nuc in "TA":
        seq, _, beg = polya_site(cfg, rng, nuc, run=30)
        for d in (120, 121):
            i0 = 300 - beg + (100 if nuc == "A" else 0)
            add(f"T1_ad{nuc}_{d}", fp, [with_sites(900, [(i0, seq), (i0 + d, seq)])], 0, n_matches=1 if d == 120 else 2,
                ad_begins_apart=(nuc, d), twin=f"T1_ad{nuc}_121" if d == 120 else None, family="T")
    # T3: two accepted positions 2 / 3 apart, the later one with the better score, so that the sort puts it first and the |delta| < 3 removal drops
    # the EARLIER one.  A third, worse TSO 121 behind the earlier position tells the two apart: 2 apart, the earlier position is gone, prev is
    # the later one and the third is only 119 / 118 behind it (one match); 3 apart, both stay, prev moves to the earlier one and the third passes.
    def t3_order(read):
        s4 = enc(read)
        lst = pm.pos_below_max(pm.scan_kmers_internal(s4, 70, len(s4) - 70, enc(tso), cfg["tso_max"], 2), cfg["tso_max"]) or []
        return [p for p, _ in lst]

    # the third: the TSO with a block of substitutions that the scan of both reads accepts and sorts behind the two positions
    for k, start in ((k, start) for k in range(cfg["tso_max"] + 2, 2, -1) for start in (8, 6, 10, 5)):
        third = tso_with_edits(cfg, k, "sub", start)
        t3 = {d: with_sites(900, [(300, dup), (300 + 121, third)]) for d, dup in T3_READS[fp].items()}
        if all(t3_order(t3[d]) == [301 + d, 301, 422] for d in (2, 3)):
            break
    for d in (2, 3):
        add(f"T3_{d}_apart", fp, [t3[d]], 0, n_matches=1 if d == 2 else 2, sorted_apart=(301, d, 422), twin="T3_3_apart" if d == 2 else None, family="T")
    # T2: prev moves on regardless: 100 + 100 keeps one; 100 + 121 keeps the third (121 behind the dropped second); 100 + 120 does not (220 behind the first)
    add("T2_100_100", fp, [with_sites(1000, [(300, tso), (400, tso), (500, tso)])], 0, n_matches=1, family="T")
    add("T2_100_120", fp, [with_sites(1000, [(300, tso), (400, tso), (520, tso)])], 0, n_matches=1, twin="T2_100_121", family="T")
    add("T2_100_121", fp, [with_sites(1000, [(300, tso), (400, tso), (521, tso)])], 0, n_matches=2, family="T")
    # T4: reverse then forward, begins 160 / 161 apart, the four kind pairs
    t_seq, _, t_beg = polya_site(cfg, rng, "T", run=30)
    a_seq, _, a_beg = polya_site(cfg, rng, "A", run=30)
    rev = {"tso": (rtso, L - 1), "ad": (a_seq, a_beg)}   # (sequence, index in it of the begin base)
    fwd = {"tso": (tso, 0), "ad": (t_seq, t_beg)}
    for rk, (rs, rb) in rev.items():
        for fk, (fs, fb) in fwd.items():
            for d in (160, 161):
                e = 420                      # 0-based index of the reverse match's begin base
                sites = [(e - rb, rs), (e + d - fb, fs)]
                n_splits = 1 if d == 160 else (rk == "ad") + (fk == "ad")
                add(f"T4_{rk}_{fk}_{d}", fp, [with_sites(1100, sites)], 0, n_matches=2, n_splits=n_splits, begins_apart=d,
                    twin=f"T4_{rk}_{fk}_161" if d == 160 else None, family="T")
    # T5: splits 99 / 100 apart: a reverse + forward TSO pair (split in its middle) and an isolated forward adapter (split 25 in front of it)
    for d in (99, 100):
        b = 400                               # 1-based begin of the reverse TSO
        x = b + 20 + d + 25                   # 1-based begin of the forward adapter
        sites = [(b - L, rtso), (b + 40 - 1, tso), (x - 1 - t_beg, t_seq)]
        add(f"T5_{d}", fp, [with_sites(1100, sites)], 0, n_matches=3, n_splits=1 if d == 99 else 2, twin="T5_100" if d == 99 else None, family="T")
    # T6 / T9 / T10: one, two and three isolated forward adapters (three splits: multi-chimeric, kept whole); one isolated TSO (no split)
    for k in (1, 2, 3):
        sites = [(300 + 300 * j - t_beg, t_seq) for j in range(k)]
        add(f"T6_adapters_{k}", fp, [with_sites(1200, sites)], 0, n_matches=k, n_splits=k if k < 3 else 0, multi=k == 3,
            twin="T6_adapters_3" if k == 2 else None, family="T")
    add("T9_tso_only", fp, [with_sites(1200, [(300, tso)])], 0, n_matches=1, n_splits=0, twin="T6_adapters_1", family="T")
    for k in (2, 3):
        add(f"T10_tsos_{k}", fp, [with_sites(1200, [(300 + 300 * j, tso) for j in range(k)])], 0, n_matches=k, n_splits=0, family="T")
    # T7: the adapter next to a stretch with k substitutions in front of its last base: the largest k that still aligns with nmis = ad_max, and k + 1
    def t7(k):
        n_ad = len(cfg["ad"])
        ad_k = cfg["ad"][:n_ad - 1 - k] + "".join("A" if c != "A" else "C" for c in cfg["ad"][n_ad - 1 - k:n_ad - 1]) + cfg["ad"][-1]
        seq, _, beg = polya_site(cfg, random.Random(7), "T", run=30, ad=ad_k)
        return place(pooled_filler(900), 400 - beg, seq)

    k = cfg["ad_max"]
    while model(t7(k + 1), fp)[2]:
        k += 1
    add("T7_nmis_at", fp, [t7(k)], 0, n_matches=1, ad_nmis=(cfg["ad_max"], True), twin="T7_nmis_over", family="T")
    add("T7_nmis_over", fp, [t7(k + 1)], 0, n_matches=0, ad_nmis=(cfg["ad_max"] + 1, False), family="T")
    # T8: two best adapter offsets 1 / 2 apart: the adapter with one / two bases inserted behind its sixth aligns with the same score at two offsets of
    # the window.  1 apart, the second is removed; 2 apart, both stay and the first is taken: either way the match starts at the FIRST offset, which a
    # kernel that shifted the other way, or took the last good offset, would move by one or two bases -- and the split with it.
    for d, ins in T8_INSERTS[fp].items():
        seq, _, beg = polya_site(cfg, random.Random(7), "T", run=30, ad=cfg["ad"][:6] + ins + cfg["ad"][6:])
        add(f"T8_{d}_apart", fp, [place(pooled_filler(900), 400 - beg, seq)], 0, n_matches=1, n_splits=1, best_offsets=d,
            twin="T8_2_apart" if d == 1 else None, differs="kept_offsets", family="T")


# the TSO with two / three of its bases doubled (3') or edited by a search with the model (5'): positions 301 and 301 + d are both accepted
T3_READS = {
    False: {2: CFG[False]["tso"][:6] + CFG[False]["tso"][4:], 3: CFG[False]["tso"][:7] + CFG[False]["tso"][4:]},
    True: {2: CFG[True]["tso"][:6] + CFG[True]["tso"][4:], 3: "CTACTACACGCCGCTCTTCCGATCT"},
}


T8_INSERTS = {False: {1: "C", 2: "GT"}, True: {1: "G", 2: "TG"}}   # found with the model: equal best scores at offsets o, o + d


def gate_ne(seq4, pat4, pos):
    """(4-mers on the diagonal, nErrors) of scan position pos"""
    return kmers_matching(seq4, pat4, pos), count_errors(needleman(pat4, seq4[pos - 1:pos - 1 + len(pat4)]))


def delta_of(ne, mx):
    return max(1, pm.jround(pm.f32(ne - pm.f32(mx))) - 1) if mx < ne else 1


def build_K(fp):
    cfg = CFG[fp]
    rng = random.Random(300 + fp)
    tso, L, mx = cfg["tso"], len(cfg["tso"]), cfg["tso_max"]
    pat4 = enc(tso)

    def decoy(over=4):
        """27 / 22 bases that pass the gate (the pattern's first 8 bases) and align far over the bound"""
        while True:
            s = tso[:8] + rnd(rng, L - 8)
            k, ne = gate_ne(enc(s), pat4, 1)
            if k >= 2 and ne > mx + over:
                return s

    # K1: a gated position far over the bound (the worst of 200 draws: it must not pass the kernels' Levenshtein bound either) d bases in front of
    # an exact TSO, in one background: the four reads differ between the two only
    cands = [tso[:8] + rnd(rng, L - 8) for _ in range(200)]
    dec = max((c for c in cands if gate_ne(enc(c), pat4, 1)[0] >= 2), key=lambda c: float(gate_ne(enc(c), pat4, 1)[1]))
    def k1_reads(i):
        return {d: place(place(pooled_filler(800), i, dec), i + d, tso) for d in (30, 31, 32, 33)}

    def quiet(i):  # nothing but the two sites passes the gate from 32 in front of the decoy to the end of the TSO
        return all([p for p in range(i - 31, i + d + L + 2) if kmers_matching(enc(r), pat4, p) >= 2] == [i + 1, i + d + 1] for d, r in k1_reads(i).items())

    i0 = next(i for i in range(300, 500, 3) if quiet(i))
    for d, read in k1_reads(i0).items():
        add(f"K1_d{d}", fp, [read], 0, n_matches=1, decoy_at=(i0 + 1, d), closure=d < 32, family="K")
    # K2: a chain of such positions every 31 bases over 300 bases, ending in an exact TSO; the same with one link of 32
    for label, links in (("31", [31] * 10), ("one32", [31] * 5 + [32] + [31] * 4)):
        read, i, chain = pooled_filler(1000), 300, []
        for step in links:
            while True:  # a decoy that the walk really visits (the bases in front of it may give a gated position that jumps over it)
                trial = place(read, i, decoy())
                seen = {p: ne for p, ne, _ in walk(enc(trial), pat4, mx, end=i + 1)}
                if i + 1 in seen and seen[i + 1] > mx:
                    break
            read = trial
            chain.append(i + 1)
            i += step
        read = place(read, i, tso)
        add(f"K2_chain_{label}", fp, [read], 0, n_matches=1, chain=(chain, i + 1), family="K")
    # K3: the skip of a gated position lands exactly on an acceptable (edited) TSO, which is found, and one position past it, which is then
    # never visited: no match.  (head, site) found by a search with the model: the head passes the gate and aligns over the bound THROUGH the
    # site behind it, so that its skip is as long as the head (on) or one longer (past).
    for label, (head, site) in K3_READS[fp].items():
        read = place(pooled_filler(800), 300, head + site + "C" * 8)
        add(f"K3_{label}", fp, [read], 0, skip=(301, 301 + len(head), label == "on"), n_matches=1 if label == "on" else 0,
            twin="K3_past" if label == "on" else None, family="K")


K3_READS = {
    False: {"on": ("AAGCAGT", "AAGCAATGGTATCAACGCAGAGTACAT"), "past": ("AAGCAG", "AAGCAATTGTATCATCGCAGAGAACAT")},
    True: {"on": ("CTACA", "CTGCAAGTAGCTCTTCCGATCA"), "past": ("CTACA", "GTAAACGACGATATTCCGATCT")},
}


def walk(seq4, pat4, max_errors, begin=70, end=None, min_kmers=2):
    """the positions scanForAdapterOrTSOseqKMERsForInternal visits that pass the gate: [(pos, nErrors, delta)] (the loop of pm.scan_kmers_internal)"""
    end = len(seq4) - 70 if end is None else end
    out, pos = [], begin
    while pos <= min(len(seq4) - len(pat4), end):
        delta = 1
        if kmers_matching(seq4, pat4, pos) >= min_kmers:
            ne = count_errors(needleman(pat4, seq4[pos - 1:pos - 1 + len(pat4)]))
            delta = delta_of(ne, max_errors)
            out.append((pos, float(ne), delta))
        pos += delta
    return out


def stretch_read(cfg, rng, k, adapters=False, last_adapter=True):
    """k polyT / polyA stretches of 20 bases in turn, 75 bases apart without adapters; with them, each stretch has its adapter and, at the first
    position of the adapter's search window, the adapter's first 12 bases once more: two positions per stretch pass the 3 x 4-mer gate"""
    fp, body = cfg["five_prime"], ""
    for j in range(k):
        nuc = "TA"[j % 2]
        if adapters:
            t_unit = cfg["ad"][:12] + rnd(rng, 5 if not fp else 3, "CG") + cfg["ad"] + rnd(rng, cfg["bc_umi"], "ACG") + "T" * 20 + "C"
            body += (t_unit if nuc == "T" else rc(t_unit)) + rnd(rng, 12, "CG")
        elif j == k - 1:
            # the last stretch has its adapter: a stretch that is lost at a cap, or a read that is handed over and redone wrongly, is a match lost
            t_unit = cfg["ad"] + rnd(rng, cfg["bc_umi"], "ACG") + "T" * 20 + "C"
            body += rnd(rng, 75 - len(t_unit), "CG") + (t_unit if nuc == "T" else rc(t_unit))
        else:
            body += "C" + nuc * 20 + "G" + rnd(rng, 53, "CG")
    return pooled_filler(300) + body + pooled_filler(300)


def build_C(fp):
    cfg = CFG[fp]
    rng = random.Random(400 + fp)
    tso, L = cfg["tso"], len(cfg["tso"])
    side = pooled_filler(480)
    # C1: 16 / 17 stretches in one read
    for k in (16, 17):
        add(f"C1_stretches_{k}", fp, [stretch_read(cfg, rng, k), side], 0, stretches=k, n_matches=1, cap="stretches_per_read", over=k == 17,
            twin="C1_stretches_17" if k == 16 else None, differs="stretches", family="C")
    # C2: 64 / 65 matches entering the split rules: five forward adapters 130 apart, then forward and reverse TSOs in turn, each orientation 122
    # apart (the TSO matches alone stay under the cap of their hand-over slot, which is a different counter)
    t_seq, _, _ = polya_site(cfg, rng, "T", run=30)
    for k in (64, 65):
        read, i = pooled_filler(5 * 130 + 61 * (k - 5) + 700), 280   # (the CPU test holds the count of matches: the oracle's, the read is long)
        for j in range(5):
            read = place(read, i, t_seq)
            i += 130
        i += 100
        for j in range(k - 5):
            read = place(read, i, tso if j % 2 == 0 else rc(tso))
            i += 61
        add(f"C2_matches_{k}", fp, [read, side], 0, n_matches=k, multi=True, cap="matches_per_read", over=k == 65,
            twin="C2_matches_65" if k == 64 else None, family="C")
    # C3: 64 / 65 accepted TSO positions of one orientation, 30 apart: accepted by the scan, dropped by the > 120 rule
    for k in (64, 65):
        read = pooled_filler(30 * k + 600)
        for j in range(k):
            read = place(read, 280 + 30 * j, tso)
        add(f"C3_accepted_{k}", fp, [read, side], 0, accepted=(False, k), n_matches=1, cap="accepted_positions", also="tso_slot", over=k == 65,
            twin="C3_accepted_65" if k == 64 else None, differs="accepted", family="C")
    # C4: 512 / 513 gated positions of one orientation (a cap of the first-generation select kernel, SMI_CHIM_A1): an exact TSO, so that the filter
    # queues the read, then the pattern's first 8 bases every 9
    base = filler(rng, 100, fp) + tso + "C" * 9 + (tso[:8] + "C") * 700
    pat4, s4 = enc(tso), enc(base)
    gated = [p for p in range(70, len(base) - L) if kmers_matching(s4, pat4, p) >= 2]
    for k in (512, 513):
        read = base[:gated[k - 1] + 70]       # scan positions 70 .. len - 70: the k-th gated position is the last one scanned
        add(f"C4_gated_{k}", fp, [read, side], 0, gated=(False, k), n_matches=1, cap="gated_per_read", cap_switch="SMI_CHIM_A1", over=k == 513,
            twin="C4_gated_513" if k == 512 else None, differs="gated", family="C")
    # C5: a tile with more than 2,048 gated positions of one orientation: N matches every base
    add("C5_tile_of_N", fp, [side, "N" * 2200, site_read(rng, fp, 700, 300, tso)], 1, gated=(False, 2200 - 139), family="C")


def build_Cq(fp):
    cfg = CFG[fp]
    rng = random.Random(500 + fp)
    tso = cfg["tso"]
    # C6a: 400 queued reads with 16 stretches each: 6,400 stretches against a queue of max(4 * 400, 4096)
    kinds = [stretch_read(cfg, rng, 16) for _ in range(4)]
    add("C6_stretch_queue", fp, [kinds[j % 4] for j in range(400)], 0, stretches=16, n_matches=1, queue=("stretch_queue", "stretches", 4096, 4), family="Cq")
    # C6b: 140 queued reads, 16 stretches each with two gated adapter positions: 2,240 stretches fit, 4,480 adapter positions pass max(8 * 140, 4096)
    kinds = [stretch_read(cfg, rng, 16, adapters=True) for _ in range(4)]
    add("C6_ad_queue", fp, [kinds[j % 4] for j in range(140)], 0, stretches=16, queue=("ad_queue", "ad_entries", 4096, 8), family="Cq")
    # C6c: sixteen reads (one workgroup of the select kernel) whose needed positions pass ONE region of the position queue, 65536 / 64 = 1024
    read = filler(rng, 70, fp) + (tso[:14] + "C") * 80 + filler(rng, 70, fp)
    add("C6_posq", fp, [read] * 16, 0, queue=("position_queue", "accepted", 1024, 48), family="Cq")


_BUILT = False


def all_cases():
    global _BUILT
    if not _BUILT:
        for fp in (False, True):
            build_S(fp)
            build_T(fp)
            build_K(fp)
            build_C(fp)
            build_Cq(fp)
        _BUILT = True
    return CASES


def by_name():
    return {c["name"]: c for c in all_cases()}


_EXPECTED = {}


def oracle_params(sor, five_prime):
    c = CFG[bool(five_prime)]
    return sor.chimera_params(tso=c["tso"], adapter=c["ad"], tso_max=c["tso_max"], adapter_max=c["ad_max"], bc_umi=c["bc_umi"])


def expected(sor, read, five_prime):
    """the oracle's (rc, splits, multi, n_matches) of one read, computed once per distinct sequence"""
    key = (read, bool(five_prime))
    if key not in _EXPECTED:
        _EXPECTED[key] = sor.chimera_split(read, oracle_params(sor, five_prime))[:4]
    return _EXPECTED[key]


def ref_exec_reads(five_prime):
    """the reads of the reference-bytecode pin (tools/make_ref_exec.py chimera_edges_*): targets only, at most 40 -- a pair per threshold of family T
    (of T4 the TSO / TSO and adapter / adapter pairs, of the adapters' 120 rule the polyT pair), the TSO bounds of S4 and one trigger pair per end, S5, K3"""
    keep = []
    for c in all_cases():
        if c["five_prime"] != bool(five_prime):
            continue
        name = c["name"][3:]
        fam = name.split("_")[0]
        if name.startswith(("T1_adA", "T4_tso_ad", "T4_ad_tso")) or name in ("T6_adapters_1", "T9_tso_only", "T2_100_100"):
            continue
        if (fam in ("T1", "T2", "T3", "T4", "T5", "T6", "T7", "T8", "S5", "K3") or name.startswith("S4_tso")
                or name in ("S4_trig_T_first", "S4_trig_T_before", "S4_trig_A_last", "S4_trig_A_after")):
            keep.append((c["name"], c["reads"][c["target"]]))
    assert len(keep) <= 40
    return keep
