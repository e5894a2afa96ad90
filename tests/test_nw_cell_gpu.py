"""The six-operation Needleman-Wunsch cell of csrc/smi_nw.h on the GPU: hand-planted read ends through the shipped and the generic K-SCAN kernels
against the oracle in pass 2 (10-mer, band 3; TSO, band 7), pass 1 (the 22-mer, band 12, whose rows 17 .. 22 use the second tag word) and the 5'
mode, and a few hundred chimeras through K-CHIM (nw_errors and the 22- / 25-mer nw_full) against the oracle.

Every end is all C (no 4-mer of the adapter or of the TSO occurs in it) but for one plant, the slices at which this cell can go wrong:
  ties      a one-base insertion or deletion next to a substitution, at every position of the pattern's middle: diagonal-mismatch, up and
            left tie in some cell, and the tag order must break the tie as the reference does
  late      a copy that starts 1 .. 5 bases late: leading template gaps (ne = #x - 0.9 * lead)
  edge      a copy shifted by exactly the band, early and late.  For the 10-mer the optimal path then runs along the band's edge (proved below);
            the TSO and the 22-mer resemble themselves too much at shifts 7 and 12 for such a path to beat the diagonal of a slice that passes
            the gate, so there the edge cells are computed and must lose
  runs      one and two substitutions in the middle (consec / best_two / nmis would show a match / mismatch swap at once)
  all N     a stretch of N under the pattern: every cell matches, the << 1 on every diagonal
  accepted  a complete adapter in front of a polyT: end5 / endn / term6 decide what the record says
The `test_planted_*` tests prove with the CPU model of the gate (tools/scan_gate_model.py) that every planted slice is a candidate, i.e. is
aligned, and with the CPU model of the cell (test_nw_cell) what its alignment looks like.  They need no GPU."""
import numpy as np
import pytest
import torch

from pymodel_scan import ENC4
from test_nw_band import nw_band
from test_nw_cell import _walk, fill6
from test_scan_gpu import AD
from test_scan_lanes_gpu import E, TSO, _batch, _codes, _put, _run_all, gm

gpu = pytest.mark.gpu     # (test_scan_lanes_gpu's module-level mark does not travel with the import)

AD10, AD22 = AD[2], AD[1]
PE = 150                  # the planted polyT runs are scan positions 110 .. 150: the adapter's gate covers 1 .. 138
P_TSO = 20                # scan position of the TSO plants
P_AD = 60                 # ... of the 10-mer plants; the 22-mer begins 12 bases earlier
OTHER = {"A": "G", "G": "A", "C": "G", "T": "G"}   # a base that is neither the pattern's nor the background's


# ---- the CPU model of one alignment --------------------------------------------------------------------------------------------------------
def _model(pat_s, sl_s, w):
    """the banded fill of the new cell and the walk over its tags -> lead, #x, largest |r - c| on the path, three-way ties in the band"""
    n = len(pat_s)
    assert len(sl_s) == n
    pat, sl = [ENC4[c] for c in pat_s], [ENC4[c] for c in sl_s]
    M = np.array([[[(sl[r] & pat[c]) != 0 for c in range(n)] for r in range(n)]])
    tags, _ = fill6(M, w)
    moves = _walk(tags[0], n)
    r = c = n
    off = 0
    for m in moves:
        off = max(off, abs(r - c))
        r, c = r - (m != "l"), c - (m != "u")
    lead = 0
    while lead < len(moves) and moves[-1 - lead] == "u":
        lead += 1
    S = [[-5 * c if r == 0 else -4 * r if c == 0 else 0 for c in range(n + 1)] for r in range(n + 1)]
    ties = 0
    for r in range(1, n + 1):
        for c in range(1, n + 1):
            d, u, le = S[r - 1][c - 1] + (5 if M[0, r - 1, c - 1] else -5), S[r - 1][c] - 5, S[r][c - 1] - 5
            S[r][c] = max(d, u, le)
            ties += d == u == le and abs(r - c) < w
    return {"lead": lead, "nx": sum(m != "m" for m in moves), "off": off, "ties": ties}


# ---- the plants ----------------------------------------------------------------------------------------------------------------------------
def _tie_variants(p):
    """an insertion and a deletion next to a substitution at every position from the sixth base on (the first five keep the gate open)"""
    out = []
    for i in range(5, len(p) - 2):
        x = OTHER[p[i]]
        out.append(("ins+sub@%d" % i, p[:i] + x + x + p[i + 1:]))
        out.append(("del+sub@%d" % i, p[:i] + x + p[i + 2:]))
    return out


def _late(p, k):
    """k other bases, then the pattern without the k bases in front of its last five, which stay on the diagonal for the gate"""
    n = len(p)
    return "".join(OTHER[p[i]] for i in range(k)) + p[:n - 5 - k] + p[n - 5:]


def _edge(p, w, late, q):
    """the pattern shifted by exactly the band, five N at q .. q + 4: they match on the diagonal (the gate) and on the shifted path alike"""
    n = len(p)
    s = [OTHER[p[i]] for i in range(w)] + list(p[:n - w]) if late else list(p[w:]) + [OTHER[p[i]] for i in range(n - w, n)]
    s[q:q + 5] = "NNNNN"
    return "".join(s)


def _sub(p, where):
    s = list(p)
    for i in where:
        s[i] = OTHER[s[i]]
    return "".join(s)


def _tso_plants():
    w = nw_band(16, 5)
    pl = [("exact", TSO), ("sub1", _sub(TSO, [8])), ("sub2", _sub(TSO, [6, 10])), ("sub2far", _sub(TSO, [5, 12]))]
    pl += _tie_variants(TSO)
    pl += [("late%d" % k, _late(TSO, k)) for k in range(1, 6)]
    pl += [("edge late", _edge(TSO, w, True, 9)), ("edge early", _edge(TSO, w, False, 2))]
    return pl


def _ad10_plants():
    """(name, what replaces the adapter's last ten bases); the twelve bases in front of them are the complete adapter's"""
    w = nw_band(10, 5)
    pl = [("exact", AD10), ("sub1", _sub(AD10, [6])), ("sub2", _sub(AD10, [5, 8])), ("sub last", _sub(AD10, [9]))]
    pl += _tie_variants(AD10)
    # (the 10-mer's own indel + substitution pairs tie nowhere inside the band; these two do: an inserted A and substitutions behind it)
    pl += [("ins+subs a", AD10[:5] + "ACACT"), ("ins+subs b", AD10[:5] + "ACGCT")]
    pl += [("late%d" % k, _late(AD10, k)) for k in range(1, 6)]
    pl += [("edge late", _edge(AD10, w, True, 1)), ("edge late 2", _edge(AD10, w, True, 3)), ("edge early", _edge(AD10, w, False, 4))]
    return pl


def _ad22_plants():
    """(name, the 22 bases at the 22-mer's position): indels and substitutions in rows 17 .. 22 come with the 10-mer plants; these are the 22-mer's own"""
    w = nw_band(22, 5)
    pl = [("sub1", _sub(AD22, [11])), ("sub2", _sub(AD22, [8, 15]))]
    pl += [v for v in _tie_variants(AD22) if 8 <= int(v[0].split("@")[1]) <= 13]
    pl += [("late%d" % k, _late(AD22, k)) for k in range(1, 6)]
    pl += [("edge late", _edge(AD22, w, True, 14)), ("edge early", _edge(AD22, w, False, 3))]
    return pl


def _c_end():
    return ["C"] * E


def _t_end():
    e = _c_end()
    _put(e, PE - 40, "T" * 41)
    return e


def _ends():
    """-> [(kind, name, end)]: one plant per end"""
    out = []
    for name, s in _tso_plants():
        e = _c_end()
        _put(e, P_TSO, s)
        out.append(("tso", name, e))
    e = _c_end()
    _put(e, 10, "N" * 30)
    out.append(("tso N", "all N", e))
    for name, s in _ad10_plants():
        e = _t_end()
        _put(e, P_AD - 12, AD22[:12] + s)
        out.append(("ad10", name, e))
    for name, s in _ad22_plants():
        e = _t_end()
        _put(e, P_AD - 12, s)
        out.append(("ad22", name, e))
    e = _t_end()
    _put(e, 30, "N" * 40)
    out.append(("ad N", "all N", e))
    return out


def _pairs(ends):
    """one read per planted end, the plant on alternating sides; the other end is all C"""
    return [(e, _c_end()) if i % 2 == 0 else (_c_end(), e) for i, (_, _, e) in enumerate(ends)]


def _slice(e, pos1, n):
    return "".join(e[pos1 - 1:pos1 - 1 + n])


def _gates(ends):
    codes = _codes([(e, e) for _, _, e in ends])[0::2]
    return (gm.gate_masks(codes, TSO, gm.TSO_WINDOW), gm.gate_masks(codes, AD10, PE - 12), gm.gate_masks(codes, AD22, PE - 12))


# ---- the plants, proved without a GPU ------------------------------------------------------------------------------------------------------
def test_planted_slices_are_candidates():
    ends = _ends()
    assert 2 * len(ends) <= 4096
    tso_m, ad10_m, ad22_m = _gates(ends)
    for i, (kind, name, e) in enumerate(ends):
        if kind == "tso":
            assert tso_m[i, P_TSO - 1], name                   # (the N of the edge plants pass the adapter's gate as well: no polyT, no adapter scan)
        elif kind == "tso N":
            assert tso_m[i, 9:24].all()                        # every position under the stretch
        elif kind == "ad10":
            assert ad10_m[i, P_AD - 1], name
        elif kind == "ad22":
            assert ad22_m[i, P_AD - 13], name
        else:
            assert ad10_m[i, 29:60].all() and ad22_m[i, 29:48].all()
        if kind.startswith("ad") and "N" not in e:
            assert not tso_m[i].any(), name                    # an adapter plant without N brings no TSO candidate along, and a T run none of either


def test_planted_alignments():
    ends = {(k, n): e for k, n, e in _ends()}
    for kind, pat, pos, w in (("tso", TSO, P_TSO, 7), ("ad10", AD10, P_AD, 3), ("ad22", AD22, P_AD - 12, 12)):
        assert w == nw_band(len(pat), 5)
        got = {n: _model(pat, _slice(e, pos, len(pat)), w) for (k, n), e in ends.items() if k == kind}
        assert sum(m["ties"] for n, m in got.items() if "+sub" in n) > 0, kind          # some cell ties three ways
        for k in range(1, 6):                                                            # leading template gaps
            if (kind, k) not in (("tso", 5), ("ad10", 3), ("ad10", 4), ("ad10", 5)):     # (there the diagonal wins: 5 > 16 - 11, 3 = the band)
                assert got["late%d" % k]["lead"] == k and got["late%d" % k]["nx"] == 2 * k, (kind, k, got["late%d" % k])
        if kind != "ad22":
            assert got["exact"] == {"lead": 0, "nx": 0, "off": 0, "ties": 0}
            assert got["sub1"]["nx"] == 1 and got["sub2"]["nx"] == 2
        if kind == "ad10":                                                               # the path runs along the edge of the band
            for n in ("edge late", "edge late 2"):
                assert got[n]["off"] == w and got[n]["lead"] == w, got[n]
    # the 10-mer plants seen by the 22-mer of pass 1: the indels sit in rows 17 .. 22, whose tags go to the second word
    for (k, n), e in ends.items():
        if k == "ad10" and "+sub" in n:
            m = _model(AD22, _slice(e, P_AD - 12, 22), 12)
            assert m["nx"] in (2, 3) and m["lead"] == 0, (n, m)


# ---- the kernels against the oracle --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    ends = _ends()
    ra, qa, offs = _batch(_pairs(ends), np.random.default_rng(7301))
    return ends, ra, qa, offs


@gpu
def test_planted_ends_pass2_and_pass1(pkg, sor, gpu_ctx, monkeypatch, batch):
    """shipped and generic kernels == oracle on every field, in pass 2 and in pass 1; and the oracle's records say the plants were found"""
    ends, ra, qa, offs = batch
    kinds = np.array([k for k, _, _ in ends])
    names = [n for _, n, _ in ends]
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)
    tso = (exp["tso_start"] != 0) | (exp["tso_end"] != 0)
    for want in ("exact", "sub1", "sub2", "late1", "late2"):   # nmis <= 4 at the planted position, and no position of the end has a smaller ne
        i = next(k for k in range(len(ends)) if kinds[k] == "tso" and names[k] == want)
        assert tso[i], want
    no_n = np.array(["N" not in e for _, _, e in ends])
    assert not tso[np.char.startswith(kinds, "ad") & no_n].any()
    found = exp["adapter_found"] == 1
    for want in ("exact", "sub1", "sub last", "late1"):
        i = next(k for k in range(len(ends)) if kinds[k] == "ad10" and names[k] == want)
        assert found[i], want
    assert not found[np.char.startswith(kinds, "tso")].any()                      # no polyT, no adapter


@gpu
@pytest.mark.parametrize("generic", [False, True])
def test_planted_ends_5p(pkg, sor, gpu_ctx, monkeypatch, batch, generic):
    """the same ends through the 5' kernels (no polyA asked for: both ends of every read are gated over positions 1 .. 110) against the oracle's 5' scan"""
    if generic:
        monkeypatch.setenv("SMI_SCAN_GENERIC", "1")
    ends, ra, qa, offs = batch
    n = offs.size - 1
    d_reads, d_quals = torch.from_numpy(ra.copy()).cuda(), torch.from_numpy(qa.copy()).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_ends = torch.zeros((28, 2 * n), dtype=torch.int32, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_qh = torch.zeros((n, 224), dtype=torch.uint8, device="cuda")
    d_qsum = torch.zeros(n, dtype=torch.int32, device="cuda")
    gpu_ctx.pack_ends_device(d_reads, d_quals, d_offs, n, d_ends, d_len, d_qh, d_qsum, five_prime=True)
    d_out = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    gpu_ctx.scan_device(d_ends, d_len, n, gpu_ctx.scan_config_5p(2, True), d_out, None, d_qh, d_qsum)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(pkg.SCAN_RESULT_DTYPE).reshape(-1)
    n_found = 0
    for i in range(n):
        seq = bytes(ra[int(offs[i]):int(offs[i + 1])]).decode()
        qual = bytes(qa[int(offs[i]):int(offs[i + 1])]).decode()
        rc, e = sor.scan_read_5p(seq, qual, AD10, max_mm=4, dont_search_polya=True)
        assert rc == 0 and got["reserved"][i] == 0
        n_found += int(e["adapter_found"])
        assert int(got["flags"][i]) == int(e["flags"]), (i, ends[i][:2], hex(int(got["flags"][i])), hex(int(e["flags"])))
        assert got["found"][i] == e["adapter_found"], (i, ends[i][:2])
        if e["adapter_found"]:
            for f in ("adapter_start", "adapter_end", "scan_end", "adapter_nmis", "reverse", "pass1_ok"):
                assert int(got[f][i]) == int(e[f]), (i, ends[i][:2], f)
    assert n_found >= 10


@gpu
@pytest.mark.parametrize("five_prime", [False, True])
def test_chimeras_equal_oracle(pkg, sor, synth, five_prime):
    """a few hundred reads with internal adapters and TSOs through K-CHIM: nw_errors (the 27- / 22-mer TSO) and nw_full (the 22- / 25-mer adapter)"""
    from test_chimera_gpu import _run

    wl = synth.make_whitelist(5000, seed=7401)
    used = synth.pick_used(wl, 50, seed=7402)
    reads = (synth.gen_reads_5p if five_prime else synth.gen_reads)(120, used, seed=7403, n_rate=0.002)
    seqs = [c[0] for c in synth.make_chimeras(reads, 300, seed=7404)]
    res, *_ = _run(pkg, pkg.Context(0), seqs, five_prime=five_prime)
    par = sor.chimera_params(tso="CTACACGACGCTCTTCCGATCT", adapter="AAGCAGTGGTATCAACGCAGAGTAC", tso_max=5, adapter_max=5, bc_umi=0) if five_prime else None
    n_split = 0
    for i, s in enumerate(seqs):
        rc, splits, multi, n_matches, _ = sor.chimera_split(s, par) if five_prime else sor.chimera_split(s)
        got = [(sor.SPLIT_REASONS[res["reason"][i][k]], int(res["pos"][i][k])) for k in range(res["n_split"][i])]
        assert rc == 0 and not (res["flags"][i] & 6), i
        assert got == splits and bool(res["flags"][i] & 1) == multi and res["n_matches"][i] == n_matches, (i, got, splits)
        n_split += len(splits) > 0
    assert n_split > 60
