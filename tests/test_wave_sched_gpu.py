"""How the waves of K-SCAN and K-BC1 get their work (resident waves that take tiles of 64 read ends / batches of 64 reads from a counter) must not
show in the results: whole `scan_result` / `bc_window` / `bc_result` records against the oracle and against each other, on batch sizes around the wave
seam (32 reads) and the former block seam (128 reads), with far fewer tiles than resident waves, on launches in a row with different sizes (the counter
between launches), on two lanes of one context at once, and on one batch scanned whole and in chunks of one tile."""
import threading

import numpy as np
import pytest
import torch

from test_bc1_wave_gpu import DS, Case, _key_list, _plant, _records, n1_member
from test_scan_gpu import AD, _compare
from test_scan_lanes_gpu import _run_all

pytestmark = pytest.mark.gpu

SCAN_SIZES = (1, 31, 32, 33, 127, 128, 129, 257)
BC_SIZES = (1, 63, 64, 65, 257)
N_POOL = 4097


def _arrays(seqs, quals):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer("".join(seqs).encode(), dtype=np.uint8), np.frombuffer("".join(quals).encode(), dtype=np.uint8), offs


class Pool3:
    """N_POOL seeded 3' generator reads as text, the oracle's pass-2 and pass-1 records of all of them (reads do not depend on each other, so the records
    of any selection are a selection of these), and `star`: a read in which the oracle finds the adapter in both passes and a TSO"""

    def __init__(self, synth, sor):
        wl = synth.make_whitelist(50_000, seed=7101)
        used = synth.pick_used(wl, 300, seed=7102)
        reads = synth.gen_reads(N_POOL, used, seed=7103, n_rate=0.003)
        self.seqs, self.quals = zip(*(synth.materialize(reads, i) for i in range(N_POOL)))
        ra, qa, offs = _arrays(self.seqs, self.quals)
        self.exp = {p: sor.scan_batch_3p(ra, qa, offs, AD[p], n_threads=8) for p in (2, 1)}
        e2, e1 = self.exp[2][1], self.exp[1][1]
        ok = (e2["adapter_found"] == 1) & (e1["adapter_found"] == 1) & ((e2["tso_start"] != 0) | (e2["tso_end"] != 0))
        assert ok.any()
        self.star = int(np.flatnonzero(ok)[0])

    def batch(self, idx):
        return _arrays([self.seqs[i] for i in idx], [self.quals[i] for i in idx])

    def sized(self, n):
        """n reads, the last of them the read with adapter and TSO"""
        return [i for i in range(N_POOL) if i != self.star][:n - 1] + [self.star]

    def check(self, got, idx, pass_no):
        st, exp = self.exp[pass_no]
        idx = np.asarray(idx)
        return _compare(got, st[idx], exp[idx], pass1=True)


@pytest.fixture(scope="module")
def pool3(synth, sor):
    return Pool3(synth, sor)


# ---- K-SCAN, 3': shipped and generic kernels, passes 2 and 1 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_sizes_3p(pkg, sor, gpu_ctx, monkeypatch, pool3, n):
    idx = pool3.sized(n)
    ra, qa, offs = pool3.batch(idx)
    exp = _run_all(pkg, sor, gpu_ctx, monkeypatch, ra, qa, offs)   # shipped == generic == oracle, passes 2 and 1; windows shipped == generic
    assert exp["adapter_found"][n - 1] == 1 and (exp["tso_start"][n - 1] != 0 or exp["tso_end"][n - 1] != 0)
    assert (exp["adapter_found"] == pool3.exp[2][1]["adapter_found"][idx]).all()


# ---- K-SCAN, 5' ---------------------------------------------------------------------------------------------------------------------------------
class Pool5:
    """258 seeded 5' generator reads as text and the oracle's records of each (--noPolyARequired, passes 2 and 1); `star`: a read whose adapter the
    oracle finds in both passes"""

    def __init__(self, synth, sor):
        n = max(SCAN_SIZES) + 1
        wl = synth.make_whitelist(50_000, seed=7201)
        used = synth.pick_used(wl, 300, seed=7202)
        reads = synth.gen_reads_5p(n, used, seed=7203, n_rate=0.003, q_mean=14.0)
        self.seqs, self.quals = zip(*(synth.materialize(reads, i) for i in range(n)))
        self.exp = {p: [sor.scan_read_5p(s, q, AD[p], max_mm=4, dont_search_polya=True) for s, q in zip(self.seqs, self.quals)] for p in (2, 1)}
        # (every 5' generator read carries the TSO behind its UMI; the 5' scan reports none, so the adapter is what the records can show)
        ok = [all(self.exp[p][i][0] == 0 and self.exp[p][i][1]["adapter_found"] for p in (2, 1)) for i in range(n)]
        assert any(ok)
        self.star = ok.index(True)
        self.n = n

    def sized(self, n):
        return [i for i in range(self.n) if i != self.star][:n - 1] + [self.star]


@pytest.fixture(scope="module")
def pool5(synth, sor):
    return Pool5(synth, sor)


def _scan_5p(pkg, ctx, ra, qa, offs, pass_no):
    n = offs.size - 1
    d_reads, d_quals = torch.from_numpy(ra.copy()).cuda(), torch.from_numpy(qa.copy()).cuda()
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    d_ends = torch.zeros((28, 2 * n), dtype=torch.int32, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_qh = torch.zeros((n, 224), dtype=torch.uint8, device="cuda")
    d_qsum = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx.pack_ends_device(d_reads, d_quals, d_offs, n, d_ends, d_len, d_qh, d_qsum, five_prime=True)
    d_out = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    d_win = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    ctx.scan_device(d_ends, d_len, n, ctx.scan_config_5p(pass_no, True), d_out, d_win, d_qh, d_qsum)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(pkg.SCAN_RESULT_DTYPE).reshape(-1), d_win.cpu()


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_sizes_5p(pkg, gpu_ctx, monkeypatch, pool5, n):
    idx = pool5.sized(n)
    ra, qa, offs = _arrays([pool5.seqs[i] for i in idx], [pool5.quals[i] for i in idx])
    for pass_no in (2, 1):
        runs = []
        for generic in (False, True):
            if generic:
                monkeypatch.setenv("SMI_SCAN_GENERIC", "1")
            else:
                monkeypatch.delenv("SMI_SCAN_GENERIC", raising=False)
            got, win = _scan_5p(pkg, gpu_ctx, ra, qa, offs, pass_no)
            runs.append((got, win))
            for k, i in enumerate(idx):
                rc, e = pool5.exp[pass_no][i]
                if rc != 0:  # the reference throws in getMeanQV: flagged, not guessed
                    assert got["reserved"][k] == 1
                    continue
                assert got["reserved"][k] == 0
                assert int(got["flags"][k]) == int(e["flags"]), (n, pass_no, generic, k)
                assert got["found"][k] == e["adapter_found"]
                assert (got["polya_start"][k], got["polya_end"][k]) == (e["polya_start"], e["polya_end"])
                if e["adapter_found"]:
                    for f in ("adapter_start", "adapter_end", "scan_end", "adapter_nmis", "reverse", "pass1_ok"):
                        assert int(got[f][k]) == int(e[f]), (n, pass_no, generic, k, f)
        monkeypatch.delenv("SMI_SCAN_GENERIC", raising=False)
        assert torch.equal(runs[0][1], runs[1][1])   # the barcode windows: shipped == generic
        assert runs[0][0]["found"][n - 1] == 1


# ---- the counter ------------------------------------------------------------------------------------------------------------------------------
class Packed:
    """a selection of the 3' pool packed on the device, with output buffers of its own"""

    def __init__(self, ctx, pool, idx):
        ra, qa, offs = pool.batch(idx)
        n = self.n = len(idx)
        self.idx = idx
        d_reads, d_quals = torch.from_numpy(ra.copy()).cuda(), torch.from_numpy(qa.copy()).cuda()
        d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
        self.d_ends = torch.zeros((28, 2 * n), dtype=torch.int32, device="cuda")
        self.d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.d_qtail = torch.zeros((n, 224), dtype=torch.uint8, device="cuda")
        self.d_qsum = torch.zeros(n, dtype=torch.int32, device="cuda")
        ctx.pack_ends_device(d_reads, d_quals, d_offs, n, self.d_ends, self.d_len, self.d_qtail, self.d_qsum)
        torch.cuda.synchronize()

    def launch(self, ctx, pass_no=2, stream=None):
        """the outputs are allocated and zeroed on the stream the scan runs on (the calling thread's current stream when none is given), so the fill
        is ordered in front of the kernel's stores; the inputs were packed and waited for in __init__"""
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            d_out = torch.zeros((self.n, 8), dtype=torch.int32, device="cuda")
            d_win = torch.zeros((self.n, 2), dtype=torch.int64, device="cuda")
            ctx.scan_device(self.d_ends, self.d_len, self.n, ctx.scan_config(pass_no), d_out, d_win, self.d_qtail, self.d_qsum)
        return d_out, d_win


def _records_of(pkg, d_out):
    return d_out.cpu().numpy().view(pkg.SCAN_RESULT_DTYPE).reshape(-1)


def test_far_fewer_tiles_than_waves(pkg, gpu_ctx, pool3):
    """33 reads are two tiles on a device that holds thousands of waves: the grid is one block, its idle waves leave, and the next launch of the same
    context finds its counter as it needs it -- twice in a row, then a batch of many tiles"""
    small, large = Packed(gpu_ctx, pool3, pool3.sized(33)), Packed(gpu_ctx, pool3, list(range(N_POOL)))
    outs = [small.launch(gpu_ctx), small.launch(gpu_ctx), large.launch(gpu_ctx), small.launch(gpu_ctx)]
    torch.cuda.synchronize()
    for b, (d_out, d_win) in zip((small, small, large, small), outs):
        assert pool3.check(_records_of(pkg, d_out), b.idx, 2) > 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][0], outs[3][0]) and torch.equal(outs[0][1], outs[3][1])


def test_counter_between_launches(pkg, gpu_ctx, pool3):
    """one context launched three times in a row with no wait between the launches: large, small, large"""
    a = Packed(gpu_ctx, pool3, list(range(N_POOL)))
    b = Packed(gpu_ctx, pool3, pool3.sized(31))
    c = Packed(gpu_ctx, pool3, list(range(N_POOL - 1, 0, -1)))
    for pass_no in (2, 1):
        outs = [x.launch(gpu_ctx, pass_no) for x in (a, b, c)]
        torch.cuda.synchronize()
        for x, (d_out, _) in zip((a, b, c), outs):
            assert pool3.check(_records_of(pkg, d_out), x.idx, pass_no) > 0


def test_two_lanes_at_once(pkg, gpu_ctx, pool3):
    """two lanes of one context scan different batches at the same time from two host threads, each on a stream of its own, several launches in a
    row: every result equals the result of the same batch scanned alone"""
    batches = [Packed(gpu_ctx, pool3, list(range(N_POOL))), Packed(gpu_ctx, pool3, list(range(N_POOL - 1, 2000, -1)) + pool3.sized(33))]
    alone = []
    for b in batches:
        d_out, d_win = b.launch(gpu_ctx)
        torch.cuda.synchronize()
        assert pool3.check(_records_of(pkg, d_out), b.idx, 2) > 0
        alone.append((d_out, d_win))
    lanes = [gpu_ctx.lane(), gpu_ctx.lane()]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    results, errors = [None, None], []
    start = threading.Barrier(2)

    def work(k):
        try:
            start.wait()
            outs = [batches[k].launch(lanes[k], stream=streams[k]) for _ in range(6)]
            streams[k].synchronize()
            results[k] = outs
        except Exception as e:  # noqa: BLE001  (reported by the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    try:
        assert not errors, errors
        for k in range(2):
            for d_out, d_win in results[k]:
                assert torch.equal(d_out, alone[k][0]) and torch.equal(d_win, alone[k][1]), k
    finally:
        for lane in lanes:
            lane.close()


def test_tile_order_does_not_matter(pkg, gpu_ctx, monkeypatch, pool3):
    """4,097 reads scanned whole == the same reads scanned in chunks of 32 (one tile to a launch), record for record and window for window"""
    whole = Packed(gpu_ctx, pool3, list(range(N_POOL)))
    d_out, d_win = whole.launch(gpu_ctx)
    outs, wins = [], []
    for r0 in range(0, N_POOL, 32):
        m = min(32, N_POOL - r0)
        o = torch.zeros((m, 8), dtype=torch.int32, device="cuda")
        w = torch.zeros((m, 2), dtype=torch.int64, device="cuda")
        gpu_ctx.scan_device(whole.d_ends[:, 2 * r0:2 * (r0 + m)].contiguous(), whole.d_len[r0:r0 + m].contiguous(), m, gpu_ctx.scan_config(2), o, w,
                            whole.d_qtail[r0:r0 + m].contiguous(), whole.d_qsum[r0:r0 + m].contiguous())
        outs.append(o)
        wins.append(w)
    torch.cuda.synchronize()
    assert torch.equal(d_out, torch.cat(outs)) and torch.equal(d_win, torch.cat(wins))
    assert pool3.check(_records_of(pkg, d_out), whole.idx, 2) > 0.3 * N_POOL


# ---- K-BC1 ------------------------------------------------------------------------------------------------------------------------------------
def test_bc1_sizes(pkg, synth, sor, gpu_ctx, monkeypatch):
    """batches of 1, 63, 64, 65 and 257 reads with the barcode itself on the last read, 3' and 5': default path == SMI_BC1_TWO_KERNELS=1 == oracle
    (test_bc1_wave_gpu.Case.check), and launches in a row of different sizes"""
    keys = _key_list(synth, 2_000)
    gpu_ctx.set_barcode_set(keys, mode=0)
    n_max = max(BC_SIZES)
    for five_prime in (False, True):
        rng = np.random.default_rng(7300 + five_prime)
        k_at = np.array([n1_member(keys[i:i + 1], (7 * i) % 169)[0] for i in range(n_max)], dtype=np.uint64)
        d_at = np.array([DS[i % 5] for i in range(n_max)])
        for m in BC_SIZES:
            k_at[m - 1], d_at[m - 1] = keys[m - 1], 0
        codes, ae = _records(_plant(k_at, d_at, rng), five_prime, rng)
        c = Case(pkg, sor, keys, codes, ae, five_prime)
        for n in BC_SIZES + (1, n_max):   # (and once more small then large: the counter between launches)
            got = c.check(pkg, gpu_ctx, monkeypatch, n)
            assert got["found"][n - 1] == 1 and got["ed"][n - 1] == 0 and got["offset"][n - 1] == 0, (five_prime, n)
