"""K-SCAN's lazily computed statistics on hand-planted waves (tests/test_scan_lazy_cpu.py builds and proves them): the rescue branch of phase C behind
its ballot, the exchange inside it, the adapter fold's ties inside a round and across a round seam, the pass-1 filter's endn == 0 -- the shipped and
the generic kernels against the oracle, passes 2 and 1."""
import importlib

import numpy as np
import pytest
import torch

from test_scan_gpu import AD, _compare
from test_scan_lanes_gpu import _batch, _run_all
from test_scan_lazy_cpu import (AD_POS, BOTH, RULE_KNOBS, TIES, both_wave, partial_wave, pass1_batch, rescue_wave, rule_wave, seam_wave, ties_5p,
                                ties_wave)
from test_scan_queue_gpu import _pairs

pytestmark = pytest.mark.gpu


def _go(pkg, sor, gpu_ctx, monkeypatch, ends, seed):
    ra, qa, offs = _batch(_pairs(ends), np.random.default_rng(seed))
    return _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs), offs


def _tso(exp):
    return np.stack([exp["tso_start"], exp["tso_end"]], 1)


@pytest.mark.parametrize("lane", [0, 63])
def test_one_lane_needs_the_rescue(pkg, sor, gpu_ctx, monkeypatch, lane):
    """wave 1: `lane` alone is present and not passed, so the whole wave enters the branch for it; wave 2: the same wave without that lane skips it"""
    exp, _ = _go(pkg, sor, gpu_ctx, monkeypatch, rescue_wave(lane) + rescue_wave(lane, with_lane=False), 7100 + lane)
    t = _tso(exp)
    rd = lane >> 1
    assert t[rd, lane & 1] != 0 and (t[32 + rd] == 0).all()          # rescued by best_two; without the lane the read has no TSO
    keep = np.arange(32) != rd
    assert (t[:32][keep] == t[32:][keep]).all() and (t[:32][keep].max(1) != 0).all()


def test_both_ends_need_the_rescue(pkg, sor, gpu_ctx, monkeypatch):
    exp, _ = _go(pkg, sor, gpu_ctx, monkeypatch, both_wave(), 7201)
    t = _tso(exp) != 0
    assert t[5].tolist() == [True, False]       # consec rescues the head, so the second rule is not asked for the tail
    assert t[9].tolist() == [True, True]        # both by best_two
    assert t[12].tolist() == [False, True]
    assert t[20].tolist() == [False, False]
    assert t[27].tolist() == [True, True]
    assert t[30].tolist() == [False, False]     # the run that starts the walk does not count
    assert t[[i for i in range(32) if i not in BOTH]].all()


def _scan_with(pkg, ctx, ra, qa, offs, cfg, five_prime=False):
    n = offs.size - 1
    d_reads, d_quals = torch.from_numpy(ra.copy()).cuda(), torch.from_numpy(qa.copy()).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_ends = torch.zeros((28, 2 * n), dtype=torch.int32, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_qtail = torch.zeros((n, 224), dtype=torch.uint8, device="cuda")
    d_qsum = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx.pack_ends_device(d_reads, d_quals, d_offs, n, d_ends, d_len, d_qtail, d_qsum, five_prime=five_prime)
    d_out = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    ctx.scan_device(d_ends, d_len, n, cfg, d_out, None, d_qtail, d_qsum)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(pkg.SCAN_RESULT_DTYPE).reshape(-1)


def test_nmis_rule_after_a_rescue(pkg, sor, gpu_ctx):
    """abs(f.nmis - r.nmis) > 3 between two rescued ends cannot happen under the shipped limits (a rescued end has 6 .. 9 mismatches); with
    maxNeedlemanMismatches 7 it does, through the generic kernels, which read the limits from the configuration"""
    lib = importlib.import_module("sicelore_amd.lib")
    k = lib.run_knobs(**RULE_KNOBS)
    par = sor.set_tso_params(sor.default_scan_params(), k.tso_scan.decode(), k.tso_scan_window, k.tso_scan_max_mm, k.tso_scan_min_consec, k.tso_scan_min_two_best)
    ra, qa, offs = _batch(_pairs(rule_wave()), np.random.default_rng(7301))
    for pass_no in (2, 1):
        got = _scan_with(pkg, gpu_ctx, ra, qa, offs, gpu_ctx.scan_config(pass_no, knobs=k))
        st, exp = sor.scan_batch_3p(ra, qa, offs, AD[pass_no], params=par, n_threads=4)
        _compare(got, st, exp, pass1=True)
    t = _tso(exp) != 0
    assert t[3].tolist() == [False, True] and t[20].tolist() == [True, False]     # the end with more mismatches was dropped


def test_no_tso_candidate_and_ties_in_one_round(pkg, sor, gpu_ctx, monkeypatch):
    """(test_planted_ties_wave: one round, no TSO candidate in the whole wave)"""
    ends, plan = ties_wave()
    exp, offs = _go(pkg, sor, gpu_ctx, monkeypatch, ends, 7401)
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    assert (_tso(exp) == 0).all()
    for rd, side, k in plan:
        assert exp["adapter_found"][rd] == 1
        assert lens[rd] - exp["adapter_start"][rd] + 1 == AD_POS[TIES[k][1]], (rd, k)


def test_tie_across_a_round_seam(pkg, sor, gpu_ctx, monkeypatch):
    exp, offs = _go(pkg, sor, gpu_ctx, monkeypatch, seam_wave(), 7501)
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    assert exp["adapter_found"].sum() == 32
    assert lens[31] - exp["adapter_start"][31] + 1 == AD_POS[2]      # the candidate of round 2 beat the incumbent of round 1


@pytest.mark.parametrize("generic", [False, True])
def test_ties_5p(pkg, sor, gpu_ctx, monkeypatch, generic):
    """the same ties through the 5' kernels (no polyA asked for: more than 64 candidates, so a seam too) against the oracle's 5' scan, read by read"""
    if generic:
        monkeypatch.setenv("SMI_SCAN_GENERIC", "1")
    ra, qa, offs = _batch(_pairs(ties_5p()), np.random.default_rng(7601))
    n = offs.size - 1
    got = _scan_with(pkg, gpu_ctx, ra, qa, offs, gpu_ctx.scan_config_5p(2, True), five_prime=True)
    n_found = 0
    for i in range(n):
        seq = bytes(ra[int(offs[i]):int(offs[i + 1])]).decode()
        qual = bytes(qa[int(offs[i]):int(offs[i + 1])]).decode()
        rc, e = sor.scan_read_5p(seq, qual, AD[2], max_mm=4, dont_search_polya=True)
        assert rc == 0 and got["reserved"][i] == 0
        n_found += int(e["adapter_found"])
        assert int(got["flags"][i]) == int(e["flags"]), (i, hex(int(got["flags"][i])), hex(int(e["flags"])))
        assert got["found"][i] == e["adapter_found"]
        if e["adapter_found"]:
            for f in ("adapter_start", "adapter_end", "scan_end", "adapter_nmis", "reverse", "pass1_ok"):
                assert int(got[f][i]) == int(e[f]), (i, f)
            k = i % len(TIES) if i < 31 else 2
            assert int(e["adapter_start"]) == AD_POS[TIES[k][1]], (i, k)    # 5': scan coordinates = stranded coordinates
    assert n_found == n


def test_pass1_pair(pkg, sor, gpu_ctx, monkeypatch):
    """(test_scan_lazy_cpu.test_pass1_pair: the oracle's pass1_ok is 1, 0 within each pair); pass 1 runs the 22-mer, pass 2 the 10-mer with qualities"""
    ra, qa, offs = pass1_batch()
    _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)


@pytest.mark.parametrize("n", [1, 33, 65])
def test_partial_tiles_rescue_on_the_last_lane(pkg, sor, gpu_ctx, monkeypatch, n):
    exp, _ = _go(pkg, sor, gpu_ctx, monkeypatch, partial_wave(n), 7700 + n)
    assert exp["tso_end"][n - 1] != 0 and exp["tso_start"][n - 1] == 0
