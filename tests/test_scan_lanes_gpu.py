"""K-SCAN's lane economy (adapter gates on the partner lane, the isolated-candidate pre-filter skipped when it cannot save an alignment round, the
bit-parallel finder over the words its window reaches, the candidate queue) on hand-built reads: the shipped kernels and the generic ones
(SMI_SCAN_GENERIC=1) against the oracle in passes 2 and 1, and against each other on the barcode windows."""
import os
import sys

import numpy as np
import pytest
import torch

from test_scan_gpu import AD, _ascii_batch, _compare, _scan_gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import scan_gate_model as gm  # noqa: E402  (the CPU model of the 4-mer gate)

pytestmark = pytest.mark.gpu

COMP = str.maketrans("ACGTN", "TGCAN")
F_T5, F_A3, F_BOTH = 1 << 11, 1 << 12, 1 << 14   # SMI_F_POLY_T_5P, SMI_F_POLY_A_3P, SMI_F_POLY_T_5P_POLY_A_3P
E = 208                                          # bases of a read end the scan looks at


def _rc(s):
    return s.translate(COMP)[::-1]


def _put(end, pos1, s):
    """write s at scan position pos1 (1-based) of a list of characters, cut at the end"""
    for k, ch in enumerate(s):
        if 0 <= pos1 - 1 + k < len(end):
            end[pos1 - 1 + k] = ch


def _plain(rng, alphabet="ACG"):
    return rng.choice(list(alphabet), E).tolist()


def _polyt_end(rng, pe, ad_at=None, frag_at=None, run_from=None, fill="ACG"):
    """an end in scan orientation whose T run ends at scan position pe; the complete adapter planted so that its last ten bases start at ad_at;
    frag_at: the adapter's last five bases on the diagonal of scan position frag_at (two matching 4-mers: a gate hit and nothing more)"""
    end = _plain(rng, fill)
    _put(end, run_from if run_from is not None else max(pe - 40, 1), "T" * (pe - (run_from if run_from is not None else max(pe - 40, 1)) + 1))
    if ad_at is not None:
        _put(end, ad_at - 12, AD[1]) if ad_at > 12 else _put(end, ad_at, AD[2])
    if frag_at is not None:
        _put(end, frag_at + 5, AD[2][5:])
    return end


def _batch(ends, rng, mid=40):
    """ends: [(head in scan orientation, tail in scan orientation)] as character lists -> ASCII reads, qualities, offsets"""
    seqs = []
    for h, t in ends:
        seqs.append("".join(h) + "".join(rng.choice(list("ACG"), mid).tolist()) + _rc("".join(t)))
    quals = ["".join(chr(33 + int(q)) for q in rng.integers(5, 35, len(s))) for s in seqs]
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer("".join(seqs).encode(), dtype=np.uint8), np.frombuffer("".join(quals).encode(), dtype=np.uint8), offs


def _codes(ends):
    """both ends of every read as the gate model's 4-bit codes [2 n, E]"""
    lut = {"A": 1, "G": 2, "C": 4, "T": 8, "N": 15}
    return np.array([[lut[c] for c in e] for pair in ends for e in pair], dtype=np.int64)


def _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs, polya=None, passes=(2, 1)):
    """shipped and generic kernels == oracle on every field test_scan_gpu._compare checks, and == each other on the barcode windows; -> the oracle's pass-2 records"""
    exp2 = None
    for pass_no in passes:
        par = None
        if polya is not None:
            par = sor.default_scan_params()
            par["polya_len"], par["polya_frac"], par["window_polya"] = polya
        st, exp = sor.scan_batch_3p(ra, qa, offs, AD[pass_no], params=par, n_threads=4)
        wins = []
        for generic in (False, True):
            if generic:
                monkeypatch.setenv("SMI_SCAN_GENERIC", "1")
            else:
                monkeypatch.delenv("SMI_SCAN_GENERIC", raising=False)
            got, d_win, _, _ = _scan_gpu(pkg, gpu_ctx, ra, qa, offs, pass_no, polya=polya)
            _compare(got, st, exp, pass1=True)
            wins.append(d_win.cpu())
        monkeypatch.delenv("SMI_SCAN_GENERIC", raising=False)
        assert torch.equal(wins[0], wins[1])
        if pass_no == 2:
            exp2 = exp
    return exp2


def _partner_reads(seed=4101):
    """96 reads = three waves of pass 2.  A: polyT on exactly one end of every read.  B: the same with a polyT run on BOTH ends of two reads (the wave
    falls back).  C: gate hits at scan positions 3, 63 .. 66, 127 .. 129, 150 of ends whose polyT ends at 76, 77, 140 and 200: the chunk
    boundaries, and last = min(pe - AD, pe - 12) on both sides of 64 and 128"""
    rng = np.random.default_rng(seed)
    ends = []
    for i in range(64):  # waves A and B
        pe = int(rng.choice([60, 75, 76, 77, 90, 120, 139, 141, 160]))
        t_end = _polyt_end(rng, pe, ad_at=pe - 40 - 29 if pe - 40 - 29 >= 1 else None, frag_at=int(rng.integers(1, max(2, pe - 45))), fill="ACGT")
        other = _plain(rng)
        if i in (40, 53):
            other = _polyt_end(rng, 100, ad_at=31)
        ends.append((t_end, other) if i % 2 == 0 else (other, t_end))
    combos = [(pe, p) for pe in (76, 77, 140, 200) for p in (3, 63, 64, 65, 66, 127, 128, 129, 150) if p <= pe]
    for i, (pe, p) in enumerate(combos):  # wave C (27) ...
        t_end = _polyt_end(rng, pe, frag_at=p, run_from=120 if pe == 200 else None)
        ends.append((t_end, _plain(rng)) if i % 2 else (_plain(rng), t_end))
    for i in range(32 - len(combos)):  # ... and five ordinary ends
        ends.append((_polyt_end(rng, 90 + i, ad_at=20 + i, fill="ACGT"), _plain(rng)))
    assert len(ends) == 96
    return ends, rng


def test_partner_gates_and_fallback(pkg, sor, gpu_ctx, monkeypatch):
    ends, rng = _partner_reads()
    ra, qa, offs = _batch(ends, rng)
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
    fl = exp["flags"].astype(np.int64)
    one = ((fl & (F_T5 | F_A3)) != 0) & ((fl & F_BOTH) == 0)
    assert one[:32].all() and one[64:].all()                              # waves A and C: one end of every read
    assert ((fl[32:64] & F_BOTH) != 0).sum() == 2 and one[32:64].sum() == 30   # wave B: two reads with both
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    pe = np.where(exp["polya_start"] != 0, lens - exp["polya_start"] + 1, 0)   # K-SCAN: polya_start = len - (pe - 1) once a side is chosen
    for want in (76, 77, 140, 175):   # (a run to 200 is cut at window + 25)
        assert (pe[64:] == want).any(), (want, sorted(set(pe[64:].tolist())))
    assert exp["adapter_found"].sum() >= 30


@pytest.mark.parametrize("n", [1, 31, 33, 65])
def test_partial_waves(pkg, synth, sor, gpu_ctx, monkeypatch, n):
    """a last wave with idle lanes (1, 31, 33 reads) and one read alone in a third wave (65): 32 reads per wave"""
    wl = synth.make_whitelist(20_000, seed=4201)
    used = synth.pick_used(wl, 100, seed=4202)
    reads = synth.gen_reads(n, used, seed=4203 + n, n_rate=0.003)
    ra, qa, offs = _ascii_batch(synth, reads, n)
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
    assert n < 10 or exp["adapter_found"].sum() > 0.5 * n


TSO = gm.TSO


def _prefilter_reads():
    """64 reads = two waves on a background no 4-mer of the TSO occurs in (both ends are all C in scan orientation: _batch reverse-complements the
    tail itself), so every gated position is planted.  Wave 1: one hit per end, 64 gated in all -- everything fits one round and the pre-filter is skipped.  Wave 2: 65, with isolated
    candidates under the bound (whole TSOs) and over it (five diagonal bases), and a chain of three candidates within 26 positions whose first has
    more than 7.5 errors, so that the scan's jump rule is in play -- here the pre-filter runs."""
    def end(hits):
        e = ["C"] * E
        for kind, p in hits:
            if kind == "tso":
                _put(e, p, TSO)
            elif kind == "five":       # TSO[0:5] on the diagonal of p
                _put(e, p, TSO[:5])
            else:                      # TSO[5:10] on the diagonal of p
                _put(e, p + 5, TSO[5:10])
        return e

    ends = []
    for i in range(32):  # wave 1: 64 ends, one hit each
        a = ("tso", 5 + i) if i < 10 else ("five", 1 + 2 * i)
        b = ("five", 70 + (i % 16)) if i % 3 else ("tso", 60 + (i % 14))
        ends.append((end([a]), end([b])))
    for i in range(32):  # wave 2: 65
        a = [("tso", 3 + i)] if i % 2 else [("five", 40 + i)]
        b = [("five", 10 + i)]
        if i == 7:
            a = [("five", 12), ("mid", 15), ("tso", 32)]   # the chain: 12 (many errors), 15 (inside its jump), 32 (a whole TSO)
            b = []
        ends.append((end(a), end(b)))
    return ends


def test_prefilter_branch(pkg, sor, gpu_ctx, monkeypatch):
    ends = _prefilter_reads()
    tm = gm.gate_masks(_codes(ends), TSO, gm.TSO_WINDOW)
    iso = gm.isolated(tm)
    per_wave = tm.reshape(2, 64, -1).sum((1, 2))
    assert per_wave.tolist() == [64, 65], per_wave          # the planted counts, by the CPU model of the gate
    assert iso.reshape(2, 64, -1).sum((1, 2))[1] >= 40       # wave 2: the filter has isolated candidates to drop ...
    chain = np.nonzero(tm[2 * (32 + 7)])[0] + 1
    assert chain.tolist() == [12, 15, 32] and not iso[2 * (32 + 7), 11] and not iso[2 * (32 + 7), 14]   # ... and a chain it must leave alone
    rng = np.random.default_rng(4301)
    ra, qa, offs = _batch(ends, rng)
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
    assert (exp["tso_start"] != 0).sum() + (exp["tso_end"] != 0).sum() >= 20     # whole TSOs were accepted


def _window_reads(seed=4401):
    """64 reads: T runs that begin at scan positions 140 .. 149 and go on to, and past, position 185; runs that end exactly at 159, 160 and 161; runs
    around the word boundaries 128 and 160 of the finder's masks"""
    rng = np.random.default_rng(seed)
    ends = []
    for start in range(140, 150):
        for stop in (170, 185, 186, 200, 208):
            ends.append(_polyt_end(rng, stop, run_from=start, ad_at=60))
    for stop in (159, 160, 161):
        for start in (100, 128, 143):
            ends.append(_polyt_end(rng, stop, run_from=start, ad_at=40))
    for start, stop in ((120, 135), (127, 142), (128, 143), (129, 160), (96, 128)):
        ends.append(_polyt_end(rng, stop, run_from=start, ad_at=30))
    assert len(ends) == 64
    return [((e, _plain(rng)) if i % 2 else (_plain(rng), e)) for i, e in enumerate(ends)], rng


@pytest.mark.parametrize("window", [150, 149, 129, 128, 97])
def test_finder_window(pkg, sor, gpu_ctx, monkeypatch, window):
    """the finder's word bounds at the shipped window (150, the largest the scan accepts with polyATlength 15: window + 25 bases of each end are cut) and
    at windows that end on and next to a word of its masks"""
    ends, rng = _window_reads()
    ra, qa, offs = _batch(ends, rng)
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs, polya=(15, 0.75, window))
    if window == 150:
        assert (exp["polya_start"] != 0).sum() >= 40


@pytest.mark.parametrize("window", [160, 161])
def test_finder_window_beyond_the_scan_region_is_refused(pkg, gpu_ctx, window):
    """windows of 160 (the largest the bit-parallel finder is built for) and 161 (which would take the generic kernels) do not reach K-SCAN at all:
    window + polyATlength + 10 must fit the 175 scanned bases of a read end, and the scan refuses them by name"""
    lib = __import__("importlib").import_module("sicelore_amd.lib")
    cfg = gpu_ctx.scan_config(2)
    cfg["window_polya"] = window
    with pytest.raises(lib.SmiError) as e:
        gpu_ctx.scan_device(torch.zeros((28, 2), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), 1, cfg,
                            torch.zeros((1, 8), dtype=torch.int32, device="cuda"))
    assert "polyA window" in str(e.value)


def test_candidate_queue(pkg, sor, gpu_ctx, monkeypatch):
    """64 reads = two waves.  Wave 1: ends with gate hits at 40 and more consecutive positions (a stretch of N matches every 4-mer) next to ends with
    none -- more than 64 adapter candidates, drained in two tiles.  Wave 2: every candidate belongs to lane 63 (the last read's tail)."""
    rng = np.random.default_rng(4501)

    def n_end(pe):
        e = _polyt_end(rng, pe, ad_at=70)
        _put(e, 5, "N" * 50)
        return e

    ends = []
    for i in range(32):
        ends.append((n_end(150), ["C"] * E) if i < 3 else ((_polyt_end(rng, 100, ad_at=30), ["C"] * E) if i % 2 else (["C"] * E, ["C"] * E)))
    for i in range(32):
        ends.append((["C"] * E, n_end(140) if i == 31 else ["C"] * E))
    codes = _codes(ends)
    am = gm.gate_masks(codes, AD[2], 138)
    assert am[0, 4:44].all() and am[:64].sum() > 64          # 40 consecutive positions on one end; two tiles in wave 1
    assert not am[1].any()
    assert am[64:127].sum() == 0 and am[127].sum() >= 40     # wave 2: lane 63 alone
    ra, qa, offs = _batch(ends, rng)
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
    assert exp["adapter_found"].sum() >= 10
