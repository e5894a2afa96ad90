"""One Context whose scratch grows, is reused at a smaller size and grows again == a fresh Context for every call.

Almost every other test makes a fresh context, and those pin the fresh context to the oracle; here each call on the reused context (its
grow-only buffers at whatever size the calls before left them) is compared with the same call on a context of its own."""
import random
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TSO = "AAGCAGTGGTATCAACGCAGAGTACAT"


def _chim(pkg, ctx, seqs, five_prime):
    import torch

    dev = torch.device("cuda:0")
    n = len(seqs)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    total = int(offs[-1])
    d_reads = torch.from_numpy(np.frombuffer("".join(seqs).encode(), dtype=np.uint8).copy()).to(dev)
    d_offs = torch.from_numpy(offs).to(dev)
    d_planes = torch.full((ctx.read_planes_words(total, n),), -1, dtype=torch.int32, device=dev)
    ctx.pack_reads_device(d_reads, d_offs, n, total, d_planes)
    d_out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    ctx.chimera_device(d_planes, d_offs, n, total, ctx.chimera_config(five_prime), d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), ctx.chimera_last_counts()


@pytest.fixture(scope="module")
def chim_batches(synth):
    """batches of 1, 65, 600, 64 and 1 reads: chimeras, the length classes of the filter, and in the 600 two reads over every cap"""
    rng = random.Random(31)
    rnd = lambda k: "".join(rng.choice("ACGT") for _ in range(k))  # noqa: E731
    reads = synth.gen_reads(300, synth.pick_used(synth.make_whitelist(5000, seed=61), 50, seed=62), seed=63, n_rate=0.002)
    pool = [c[0] for c in synth.make_chimeras(reads, 731 - 17, seed=64)]
    classes = [rnd(L) for L in (1, 239, 240, 440, 441)]
    over = [rnd(150) + "".join(TSO + rnd(rng.randrange(95, 140)) for _ in range(90)) + rnd(150), "N" * 600]
    batches, at = [], 0
    for n in (1, 65, 600, 64, 1):
        extra = classes + (over if n == 600 else []) if n > 1 else []
        batches.append(extra + pool[at:at + n - len(extra)])
        at += n - len(extra)
        assert len(batches[-1]) == n
    return batches


@pytest.mark.parametrize("a1", [False, True], ids=["default", "SMI_CHIM_A1"])
def test_k_chim_on_a_reused_context_equals_fresh_contexts(pkg, chim_batches, monkeypatch, a1):
    if a1:
        monkeypatch.setenv("SMI_CHIM_A1", "1")
    reused = pkg.Context(0)
    seen_serial = 0
    for five_prime in (False, True):
        for seqs in chim_batches:
            got, got_counts = _chim(pkg, reused, seqs, five_prime)
            fresh = pkg.Context(0)
            exp, exp_counts = _chim(pkg, fresh, seqs, five_prime)
            fresh.close()
            assert (got == exp).all(), (five_prime, len(seqs))
            assert got_counts == exp_counts, (five_prime, len(seqs))
            seen_serial += got_counts["serial"]
    assert seen_serial >= 2  # the over-cap reads went through the second chance to K-CHIM-S: its buffers were allocated
    reused.close()


def test_k_chim_after_close_and_re_create(pkg, chim_batches):
    seqs = chim_batches[2]
    out = []
    for _ in range(2):
        ctx = pkg.Context(0)
        out.append(_chim(pkg, ctx, seqs, False))
        ctx.close()
    assert (out[0][0] == out[1][0]).all() and out[0][1] == out[1][1]


@pytest.fixture(scope="module")
def chunk_texts(synth):
    used = synth.pick_used(synth.make_whitelist(5000, seed=71), 40, seed=72)
    reads = synth.gen_reads(2000, used, seed=73)
    rec = lambda i, s, q: f"@r{i} x\n{s}\n+\n{q}\n"  # noqa: E731
    short = [synth.materialize(reads, i) for i in range(2000)]
    text = lambda k: "".join(rec(i, *short[i]) for i in range(k)).encode()  # noqa: E731
    # longer reads: the arena grows behind the uploaded text.  Every section of the arena is sized by the text's bytes or its record count; 2,000 records of
    # two to four molecules are at least twice the bytes of the 2,000 single molecules before them, and the arena was grown with a quarter to spare
    chim = synth.make_chimeras(reads, 2000, seed=74, parts=(2, 3, 4))
    long_text = "".join(rec(i, c[0], c[1]) for i, c in enumerate(chim)).encode()
    return used, [(text(3), False), (text(2000), False), (text(40), False), (long_text, True)]


def _chunks(pkg, used, texts, worker_of):
    """every text through worker_of(owner) on one owner context and through a fresh context each"""
    keys = used.numpy().astype(np.uint64)
    owner = pkg.Context(0)
    owner.set_barcode_set(keys, mode=0)
    worker = worker_of(owner)
    for text, split in texts:
        got = worker.scanfastq_pass2_chunk(text, split_chimeras=split)
        fresh = pkg.Context(0)
        fresh.set_barcode_set(keys, mode=0)
        exp = fresh.scanfastq_pass2_chunk(text, split_chimeras=split)
        fresh.close()
        assert bytes(got[0]) == bytes(exp[0]) and bytes(got[1]) == bytes(exp[1]) and got[2] == exp[2], (len(text), split)
        assert got[2]["n_records_in"] == text.count(b"\n") // 4
    assert len(texts[3][0]) > 2 * len(texts[1][0])  # (what the last text's growth of the arena rests on)
    if worker is not owner:
        worker.close()
    owner.close()


def test_chunk_worker_on_a_reused_context_equals_fresh_contexts(pkg, chunk_texts):
    _chunks(pkg, *chunk_texts, worker_of=lambda owner: owner)


def test_chunk_worker_on_a_reused_lane_equals_fresh_contexts(pkg, chunk_texts):
    _chunks(pkg, *chunk_texts, worker_of=lambda owner: owner.lane())


def test_index_write_index_share_one_scratch(pkg):
    """The indexer and K-WRITE share one scratch buffer: K-WRITE regrows and overwrites it, and the index of the same text (same address)
    afterwards equals the one before.  This covers the regrow and the reuse of the buffer only.  The sweep's flags are not at stake here:
    no public entry point leaves them valid (launch_fastq_index ends them itself), so that whoever takes the buffer ends them, which
    take_scan_tmp() is for, is a property of the code that no call sequence of today can show."""
    import torch

    dev = torch.device("cuda:0")
    rng = random.Random(41)
    rnd = lambda k: "".join(rng.choice("ACGT") for _ in range(k))  # noqa: E731
    lens = [rng.randrange(40, 90) for _ in range(300)]
    lens[150] = 5000
    text = torch.from_numpy(np.frombuffer("".join(f"@r{i}\n{rnd(L)}\n+\n{'5' * L}\n" for i, L in enumerate(lens)).encode(), dtype=np.uint8).copy()).to(dev)
    n, cap = len(lens), len(lens) + 2
    z64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)  # noqa: E731
    z32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)  # noqa: E731
    ctx = pkg.Context(0)

    def index():
        b = dict(line=z64(4 * cap + 8), ns=z64(cap), nl=z32(cap), ss=z64(cap), sl=z32(cap), qs=z64(cap), offs=z64(cap + 1))
        got = ctx.fastq_index_device(text, text.numel(), b["line"], b["ns"], b["nl"], b["ss"], b["sl"], b["qs"], b["offs"], cap)
        torch.cuda.synchronize()
        return got, b

    first, b = index()
    assert first == (n, 0) and b["sl"][:n].cpu().tolist() == lens
    total = int(b["offs"][n])
    bstart, qstart = z64(n), z64(n)
    ctx.frag_text_starts_device(b["ss"], b["qs"], b["offs"], None, None, n, bstart, qstart)
    scan, bc = torch.zeros((n, 8), dtype=torch.int32, device=dev), torch.zeros((n, 4), dtype=torch.int32, device=dev)
    capw = 2 * total + text.numel() + 320 * n
    out_p, out_f = torch.empty(capw, dtype=torch.uint8, device=dev), torch.empty(capw, dtype=torch.uint8, device=dev)
    bp, bf, n_p = ctx.fastq_write_device(text, b["line"], bstart, qstart, b["offs"][:n + 1], None, None, scan, bc, None, n, 1, out_p, out_f,
                                         z64(n + 1), torch.zeros(n, dtype=torch.uint8, device=dev), in_text=True)
    assert bp + bf > total  # every record is written to one of the two streams
    second, b2 = index()
    assert second == first
    for k in b:
        assert bool((b[k] == b2[k]).all()), k
    ctx.close()


def test_gzip_device_on_a_reused_context_equals_fresh_contexts(pkg):
    import torch

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    letters = np.frombuffer(b"ACGTN\n", dtype=np.uint8)
    reused = pkg.Context(0)
    for n in (100, 3_000_000, 100):
        data = letters[rng.integers(0, letters.size, n)]
        d_in = torch.from_numpy(data.copy()).to(dev)
        got = bytes(reused.gzip_device(d_in).cpu().numpy())
        fresh = pkg.Context(0)
        exp = bytes(fresh.gzip_device(d_in).cpu().numpy())
        fresh.close()
        assert got == exp, n
        assert zlib.decompress(got, 31) == data.tobytes(), n
    reused.close()


def _umi(pkg, ctx, packed, sizes):
    import torch

    dev = torch.device("cuda:0")
    sizes = np.asarray(sizes, dtype=np.int64)
    go = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    mo = np.concatenate([[0], np.cumsum(sizes * sizes)]).astype(np.uint64)
    mat = ctx.umi_dist_batch(packed, go)
    n = int(go[-1])
    d_out, d_sk = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    d_qv = torch.from_numpy((8 + (np.arange(n) * 7919 % 170) / 10).astype(np.float32)).to(dev)
    ctx.umi_cluster_groups_device(torch.from_numpy(mat.copy()).to(dev), torch.from_numpy(mo.view(np.int64)).to(dev), torch.from_numpy(go.view(np.int32)).to(dev),
                                  len(sizes), d_qv, d_out, d_sk)
    torch.cuda.synchronize()
    return mat, d_out.cpu().numpy(), d_sk.cpu().numpy()


def test_k_umi_on_a_reused_context_equals_fresh_contexts(pkg):
    rng = np.random.default_rng(11)

    def windows(sizes):
        w = []
        for m in sizes:
            base = rng.choice([1, 2, 4, 8], size=14)
            for _ in range(m):
                v = base.copy()
                for p in rng.integers(0, 14, rng.integers(0, 3)):
                    v[p] = rng.choice([1, 2, 4, 8, 15])
                w.append(sum(int(c) << (4 * k) for k, c in enumerate(v)))
        return np.array(w, dtype=np.uint64)

    reused = pkg.Context(0)
    for sizes in ([2], [150, 48] + [49] * 98, [2]):  # 2, 5,000 and 2 windows; the group of 150 is clustered on its matrix in device memory
        packed = windows(sizes)
        got = _umi(pkg, reused, packed, sizes)
        fresh = pkg.Context(0)
        exp = _umi(pkg, fresh, packed, sizes)
        fresh.close()
        for g, e in zip(got, exp):
            assert (g == e).all(), sum(sizes)
    reused.close()
