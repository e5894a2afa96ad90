"""K-SCAN's candidate numbering (the wave prefix sum through DPP, owners pushing (lane, position) into the slots of their candidates in the three
queue loops: the pre-filter's bound loop, the adapter rounds, the TSO rounds) on hand-built waves: the shipped and the generic kernels against the
oracle in passes 2 and 1.  Every wave is planted on a background on which neither gate fires (all C), and the CPU model of the gate
(tools/scan_gate_model.py) proves the planted counts first -- those proofs are the `test_planted_*` tests, which need no GPU."""
import numpy as np
import pytest
import torch

from test_scan_gpu import AD
from test_scan_lanes_gpu import E, TSO, _batch, _codes, _put, _run_all, gm

gpu = pytest.mark.gpu     # (test_scan_lanes_gpu's module-level mark does not travel with the import)

PE = 150                  # where the planted polyT runs end: the 10-mer's gate then covers scan positions 1 .. PE - 12
FIVE = AD[2][5:]          # the adapter's last five bases: two matching 4-mers on the diagonal, a gate hit and nothing more


# ---- builders ----------------------------------------------------------------------------------------------------------------------------
def _c_end():
    return ["C"] * E


def _ad_end(hits, pe=PE, run_from=None, n_run=None):
    """an all-C end whose T run ends at scan position pe, one adapter gate hit at every position of `hits` (the complete adapter where there is room
    for it, its last five bases otherwise); n_run = (position, length): a stretch of N (every 4-mer matches: one gate hit per position)"""
    e = _c_end()
    start = run_from if run_from is not None else pe - 40
    _put(e, start, "T" * (pe - start + 1))
    _ad_hits(e, hits)
    if n_run:
        _put(e, n_run[0], "N" * n_run[1])
    return e


def _ad_hits(e, hits):
    for k, p in enumerate(hits):
        if p > 12 and (k == 0 or p - hits[k - 1] >= 22):
            _put(e, p - 12, AD[1])      # the complete adapter, its last ten bases at p: one hit of the 10-mer's gate, and one of the 22-mer's
        else:
            _put(e, p + 5, FIVE)
    return e


def _tso_hits(e, hits):
    """TSO gate hits on an end: ("tso", p) a whole TSO at p (accepted; isolated when alone), ("five", p) its first five bases (a gate hit with
    too many errors for the bound: the pre-filter drops it when it is isolated), ("mid", p) bases 5 .. 9 on the diagonal of p"""
    for kind, p in hits:
        if kind == "tso":
            _put(e, p, TSO)
        elif kind == "five":
            _put(e, p, TSO[:5])
        else:
            _put(e, p + 5, TSO[5:10])
    return e


def _pairs(ends):
    """64 ends per wave in lane order -> [(head, tail)] per read"""
    assert len(ends) % 2 == 0
    return [(ends[i], ends[i + 1]) for i in range(0, len(ends), 2)]


def _ad_counts(ends, pes):
    """adapter candidates per end by the CPU model: the pass-2 gate over positions 1 .. pe - 12 of the ends that have a polyT (pes[i] > 0)"""
    codes = _codes(_pairs(ends))
    out = []
    for i, pe in enumerate(pes):
        out.append(gm.gate_masks(codes[i:i + 1], AD[2], pe - 12)[0] if pe else np.zeros(0, dtype=bool))
    return out


def _tso_masks(ends):
    return gm.gate_masks(_codes(_pairs(ends)), TSO, gm.TSO_WINDOW)


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)])


def _rounds(x):
    return (x + 63) // 64


def _takes_prefilter(tm):
    """the kernel's rule for one wave: the pre-filter runs when dropping every isolated candidate would save a round"""
    total, iso = int(tm.sum()), int(gm.isolated(tm).sum())
    return iso > 0 and _rounds(total) > _rounds(total - iso)


def _spread(n, first=3, step=24):
    return [first + step * k for k in range(n)]


def _ad_spread(n):
    """up to six adapter hits in front of a T run that begins at PE - 40: a complete adapter at 14, five-base hits from 36 on"""
    return ([14] + [36 + 15 * k for k in range(n - 1)])[:n]


def _one_side(per, end_of):
    """32 owners, one per read and on alternating sides (so that a side is chosen and the record shows the alignment) -> 64 ends, their polyT ends"""
    assert len(per) == 32
    ends, pes = [], []
    for i, n in enumerate(per):
        own = end_of(i, n)
        ends += [own, _c_end()] if i % 2 == 0 else [_c_end(), own]
        pes += [PE, 0] if i % 2 == 0 else [0, PE]
    return ends, pes


# ---- the planted waves -------------------------------------------------------------------------------------------------------------------
def _adapter_seam(total):
    """one wave with `total` adapter candidates, a polyT on one end of every read.  64 / 65: two candidates on each of 31 owners and 2 / 3 on the last
    (62 .. 64 one end).  128 / 129: four each, but two on owner 15 and five on owner 16 (numbers 62 .. 66), and 5 / 6 on the last (123 .. 128)"""
    per = [2] * 31 + [total - 62] if total <= 65 else [4] * 15 + [2, 5] + [4] * 14 + [total - 123]
    assert sum(per) == total
    return _one_side(per, lambda i, n: _ad_end(_ad_spread(n)))


def _check_adapter_seam(total):
    ends, pes = _adapter_seam(total)
    cnt = [int(m.sum()) for m in _ad_counts(ends, pes)]
    assert sum(cnt) == total, cnt
    off = _offsets(cnt)
    owner_of = lambda x: int(np.searchsorted(off, x, side="right") - 1)   # noqa: E731
    if total == 64:
        assert owner_of(62) == owner_of(63)                           # the round ends with its last owner
    elif total == 65:
        assert owner_of(62) == owner_of(64)                           # 62 .. 64 one end: the seam inside an owner
    else:
        assert owner_of(62) == owner_of(66)                           # 62 .. 66 one end
        assert owner_of(123) == owner_of(total - 1)                   # ... and the last end holds 123 .. 127 / 128
    assert not _tso_masks(ends).any()
    return ends


def _tso_seam(total):
    """one wave with `total` TSO candidates and no adapter candidate.  64: one whole TSO on 62 ends and a chain of two on end 62 (numbers 62, 63) -- the
    chain's first is not isolated, so even without the 63 isolated ones a round is needed: the pre-filter is skipped.  65 / 128 / 129: whole TSOs (isolated, under the bound: the filter runs and keeps them); one end carries a chain of five at a spacing of 17
    (numbers 62 .. 66)"""
    if total == 64:
        per = [1] * 62 + [2, 0]
    elif total == 65:
        per = [2] * 31 + [3] + [0] * 32
    else:
        per = [2] * 31 + [5] + [2] * 29 + [1, 1, total - 127]
    ends = []
    for n in per:
        pos = _spread(n, 3, 17) if n > 2 or total == 64 else _spread(n, 3, 40)   # one, or two 40 apart: isolated; 17 apart: a chain
        ends.append(_tso_hits(_c_end(), [("tso", p) for p in pos]))
    return ends, per


def _check_tso_seam(total):
    ends, per = _tso_seam(total)
    tm = _tso_masks(ends)
    assert tm.sum(1).tolist() == per and tm.sum() == total
    assert _takes_prefilter(tm) == (total != 64)
    if total > 65:
        off = _offsets(per)
        assert off[31] == 62 and off[32] == 67
    return ends


def _three_chunks():
    """one owner (lane 5) whose T run goes on to position 200 (cut at 175: the gate covers 1 .. 163) with hits in all three 64-bit chunks of its mask, among
    ordinary owners"""
    ends, pes = [], []
    for i in range(32):
        if i == 2:
            ends += [_c_end(), _ad_end([10, 40, 70, 100, 126, 135], pe=200, run_from=146)]
            pes += [0, 175]
        else:
            ends += [_ad_end(_ad_spread(i % 3)), _c_end()]
            pes += [PE, 0]
    return ends, pes


def _check_three_chunks():
    ends, pes = _three_chunks()
    m = _ad_counts(ends, pes)
    hits = (np.nonzero(m[5])[0] + 1).tolist()
    assert hits == [10, 40, 70, 100, 126, 135], hits
    assert sum(p <= 64 for p in hits) and sum(64 < p <= 128 for p in hits) and sum(p > 128 for p in hits)
    return ends, pes


def _every_end_one():
    """every end of the wave has exactly one TSO candidate, a whole TSO (all isolated: the filter runs and keeps every one)"""
    return [_tso_hits(_c_end(), [("tso", 1 + (7 * i) % 75)]) for i in range(64)]


def _check_every_end_one():
    ends = _every_end_one()
    tm = _tso_masks(ends)
    assert (tm.sum(1) == 1).all() and gm.isolated(tm).sum() == 64 and _takes_prefilter(tm)
    return ends


def _one_lane(lane):
    """only `lane` has candidates: three adapter hits and two TSO hits"""
    ends = [_c_end() for _ in range(64)]
    ends[lane] = _tso_hits(_ad_end([50, 75, 100]), [("tso", 4), ("five", 40)])
    return ends


def _check_one_lane(lane):
    ends = _one_lane(lane)
    pes = [PE if i == lane else 0 for i in range(64)]
    cnt = [int(m.sum()) for m in _ad_counts(ends, pes)]
    tm = _tso_masks(ends)
    assert [i for i in range(64) if cnt[i]] == [lane] and cnt[lane] == 3
    assert np.nonzero(tm.sum(1))[0].tolist() == [lane] and tm[lane].sum() == 2
    return ends


def _counts_0123():
    """adapter counts 0, 1, 2, 3, 0, ... along the 32 owners and TSO counts 3, 2, 1, 0, 3, ... along the 64 ends: all partial sums distinct"""
    ends, pes = _one_side([i % 4 for i in range(32)], lambda i, n: _ad_end([40 + 24 * k for k in range(n)]))
    for i, e in enumerate(ends):
        _tso_hits(e, [("tso" if k == 0 else "five", 2 + 18 * k) for k in range(3 - i % 4)])
    return ends, pes


def _check_counts_0123():
    ends, pes = _counts_0123()
    cnt = [int(m.sum()) for m in _ad_counts(ends, pes)]
    assert [c for c, p in zip(cnt, pes) if p] == [i % 4 for i in range(32)], cnt
    assert _tso_masks(ends).sum(1).tolist() == [3 - i % 4 for i in range(64)]
    return ends


def _n_end():
    e = _c_end()
    _put(e, 5, "N" * 70)
    return e


def _dense():
    """reads 0 and 1: a stretch of 70 N on BOTH ends (every position of it gated: > 128 TSO candidates, three rounds), one of the two with a polyT behind it
    (> 64 adapter candidates on two owners); the other ends carry isolated five-base TSO hits, so the packed prefix sum has large low halves beside
    non-zero high halves"""
    ends = [_ad_end([], n_run=(5, 70)), _n_end(), _n_end(), _ad_end([], n_run=(5, 70))]
    for i in range(2, 32):
        ends += [_tso_hits(_ad_end(_ad_spread(i % 2)), [("five", 30)]), _tso_hits(_c_end(), [("five", 8 + i)])]
    return ends


def _check_dense():
    ends = _dense()
    pes = [PE, 0, 0, PE] + [PE, 0] * 30
    ad = _ad_counts(ends, pes)
    cnt = [int(m.sum()) for m in ad]
    tm = _tso_masks(ends)
    run = lambda row: max(len(x) for x in "".join("1" if b else "0" for b in row).split("0"))   # noqa: E731
    assert all(run(tm[i]) >= 40 for i in range(4)) and run(ad[0]) >= 40 and run(ad[3]) >= 40
    assert tm.sum() > 128 and sum(cnt) > 64
    assert gm.isolated(tm)[4:].sum() >= 50 and _takes_prefilter(tm)
    return ends


def _many_isolated():
    """two isolated five-base hits on every end = 128 isolated candidates: the bound loop runs two rounds.  Read 7's head carries a chain inside a jump
    instead (12: many errors; 15: inside its jump; 32: a whole TSO), which the filter must leave alone"""
    ends = []
    for i in range(64):
        ends.append(_tso_hits(_c_end(), [("five", 2 + i % 20), ("five", 50 + i % 25)]))
    ends[14] = _tso_hits(_c_end(), [("five", 12), ("mid", 15), ("tso", 32)])
    return ends


def _check_many_isolated():
    ends = _many_isolated()
    tm = _tso_masks(ends)
    iso = gm.isolated(tm)
    assert iso.sum() > 64 and iso.sum() >= 126 and _takes_prefilter(tm)
    assert (np.nonzero(tm[14])[0] + 1).tolist() == [12, 15, 32] and not iso[14, 11] and not iso[14, 14]
    return ends


def _one_kind(kind):
    """a wave with TSO candidates and no adapter candidate ("tso"), and the reverse ("adapter")"""
    if kind == "tso":
        return [_tso_hits(_c_end(), [("tso", 3 + i % 30)] + ([("five", 60)] if i % 3 == 0 else [])) for i in range(64)]
    ends = []
    for i in range(32):
        ends += [_ad_end(_ad_spread(1 + i % 4)), _c_end()]
    return ends


def _check_one_kind(kind):
    ends = _one_kind(kind)
    pes = [0] * 64 if kind == "tso" else [PE, 0] * 32
    n_ad, n_ts = sum(int(m.sum()) for m in _ad_counts(ends, pes)), int(_tso_masks(ends).sum())
    assert (n_ad == 0 and n_ts > 64) if kind == "tso" else (n_ad > 64 and n_ts == 0)
    return ends


def _partial(n):
    """n reads; the last read's tail (the last active lane) has four adapter and three TSO candidates, a few owners before it one or two"""
    ends = []
    for i in range(n):
        ends += [_tso_hits(_c_end(), [("five", 20)] if i % 2 else []), _c_end()] if i < n - 1 else [_c_end(), _tso_hits(_ad_end([50, 70, 90, 110]), [("tso", 2), ("tso", 19), ("five", 70)])]
        if i % 5 == 1 and i < n - 1:
            ends[-2] = _ad_end([30, 100])
    return ends


def _check_partial(n):
    ends = _partial(n)
    pes = [0] * (2 * n)
    pes[-1] = PE
    for i in range(n - 1):
        if i % 5 == 1:
            pes[2 * i] = PE
    cnt = [int(m.sum()) for m in _ad_counts(ends, pes)]
    tm = _tso_masks(ends)
    assert cnt[-1] == 4 and tm[-1].sum() == 3 and all(c == 2 for c, p in zip(cnt[:-1], pes[:-1]) if p)
    return ends


def _seam_5p():
    """the 5' scan with no polyA asked for gates both ends of every read over positions 1 .. 110: one end of every read carries two hits, the last three (62 .. 64)"""
    per = [2] * 31 + [3]
    ends = []
    for i, n in enumerate(per):
        own = _ad_hits(_c_end(), _spread(n, 30, 24))
        ends += [own, _c_end()] if i % 2 == 0 else [_c_end(), own]
    return ends, [n for i, n in enumerate(per) for n in ((n, 0) if i % 2 == 0 else (0, n))]


def _check_seam_5p():
    ends, per = _seam_5p()
    am = gm.gate_masks(_codes(_pairs(ends)), AD[2], 110)
    assert am.sum(1).tolist() == per and am.sum() == 65
    return ends


# ---- the counts, proved without a GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [64, 65, 128, 129])
def test_planted_adapter_seam(total):
    _check_adapter_seam(total)


@pytest.mark.parametrize("total", [64, 65, 128, 129])
def test_planted_tso_seam(total):
    _check_tso_seam(total)


def test_planted_three_chunks():
    _check_three_chunks()


@pytest.mark.parametrize("lane", [0, 63])
def test_planted_one_lane(lane):
    _check_one_lane(lane)


def test_planted_every_end_one():
    _check_every_end_one()


def test_planted_counts_0123():
    _check_counts_0123()


def test_planted_dense():
    _check_dense()


def test_planted_many_isolated():
    _check_many_isolated()


@pytest.mark.parametrize("kind", ["tso", "adapter"])
def test_planted_one_kind(kind):
    _check_one_kind(kind)


@pytest.mark.parametrize("n", [1, 33, 65])
def test_planted_partial(n):
    _check_partial(n)


def test_planted_seam_5p():
    _check_seam_5p()


# ---- the kernels against the oracle ------------------------------------------------------------------------------------------------------
def _go(pkg, sor, gpu_ctx, monkeypatch, ends, seed):
    rng = np.random.default_rng(seed)
    ra, qa, offs = _batch(_pairs(ends), rng)
    return _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs), offs


def _pe_of(exp, offs):
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    return np.where(exp["polya_start"] != 0, lens - exp["polya_start"] + 1, 0)   # K-SCAN: polya_start = len - (pe - 1) once a side is chosen


@gpu
@pytest.mark.parametrize("total", [64, 65, 128, 129])
def test_adapter_round_seams(pkg, sor, gpu_ctx, monkeypatch, total):
    exp, offs = _go(pkg, sor, gpu_ctx, monkeypatch, _check_adapter_seam(total), 5100 + total)
    pe = _pe_of(exp, offs)
    assert set(pe[pe != 0].tolist()) == {PE}       # the finder ends the planted runs where the counts above assume
    assert exp["adapter_found"].sum() == 32        # every owner carries a complete adapter: a wrong owner or position loses it


@gpu
@pytest.mark.parametrize("total", [64, 65, 128, 129])
def test_tso_round_seams(pkg, sor, gpu_ctx, monkeypatch, total):
    exp, _ = _go(pkg, sor, gpu_ctx, monkeypatch, _check_tso_seam(total), 5200 + total)
    assert (exp["polya_start"] == 0).all()


@gpu
def test_three_chunks_of_one_owner(pkg, sor, gpu_ctx, monkeypatch):
    ends, _ = _check_three_chunks()
    exp, offs = _go(pkg, sor, gpu_ctx, monkeypatch, ends, 5301)
    assert _pe_of(exp, offs)[2] == 175             # (a run to 200 is cut at window + 25)


@gpu
@pytest.mark.parametrize("lane", [0, 63])
def test_one_lane_owns_everything(pkg, sor, gpu_ctx, monkeypatch, lane):
    _go(pkg, sor, gpu_ctx, monkeypatch, _check_one_lane(lane), 5400 + lane)


@gpu
def test_every_end_one_tso_candidate(pkg, sor, gpu_ctx, monkeypatch):
    exp, _ = _go(pkg, sor, gpu_ctx, monkeypatch, _check_every_end_one(), 5501)
    assert (exp["tso_start"] != 0).sum() + (exp["tso_end"] != 0).sum() >= 32


@gpu
def test_counts_0123(pkg, sor, gpu_ctx, monkeypatch):
    _go(pkg, sor, gpu_ctx, monkeypatch, _check_counts_0123(), 5601)


@gpu
def test_dense_owners_three_rounds(pkg, sor, gpu_ctx, monkeypatch):
    _go(pkg, sor, gpu_ctx, monkeypatch, _check_dense(), 5701)


@gpu
def test_prefilter_two_bound_rounds(pkg, sor, gpu_ctx, monkeypatch):
    exp, _ = _go(pkg, sor, gpu_ctx, monkeypatch, _check_many_isolated(), 5801)
    assert exp["tso_start"][7] != 0 or exp["tso_end"][7] != 0      # the whole TSO behind the chain was reached


@gpu
@pytest.mark.parametrize("kind", ["tso", "adapter"])
def test_one_kind_empty(pkg, sor, gpu_ctx, monkeypatch, kind):
    _go(pkg, sor, gpu_ctx, monkeypatch, _check_one_kind(kind), 5901)


@gpu
@pytest.mark.parametrize("n", [1, 33, 65])
def test_partial_tiles_last_lane(pkg, sor, gpu_ctx, monkeypatch, n):
    _go(pkg, sor, gpu_ctx, monkeypatch, _check_partial(n), 6000 + n)


@gpu
@pytest.mark.parametrize("generic", [False, True])
def test_seam_5p(pkg, sor, gpu_ctx, monkeypatch, generic):
    """65 adapter candidates through the 5' kernels (no polyA asked for: both ends of every read are gated) against the oracle's 5' scan, read by read"""
    if generic:
        monkeypatch.setenv("SMI_SCAN_GENERIC", "1")
    ends = _check_seam_5p()
    ra, qa, offs = _batch(_pairs(ends), np.random.default_rng(6101))
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
        rc, e = sor.scan_read_5p(seq, qual, AD[2], max_mm=4, dont_search_polya=True)
        if rc != 0:
            assert got["reserved"][i] == 1
            continue
        assert got["reserved"][i] == 0
        n_found += int(e["adapter_found"])
        assert int(got["flags"][i]) == int(e["flags"]), (i, hex(int(got["flags"][i])), hex(int(e["flags"])))
        assert got["found"][i] == e["adapter_found"]
        if e["adapter_found"]:
            for f in ("adapter_start", "adapter_end", "scan_end", "adapter_nmis", "reverse", "pass1_ok"):
                assert int(got[f][i]) == int(e[f]), (i, f)
    assert n_found == n                            # every read carries one complete adapter
