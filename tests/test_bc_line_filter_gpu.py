"""K-BC1's line filter `nbl` on the GPU: the folded table holds what a numpy model of the barcodes' 169-slot neighbourhoods says, and the matcher's
records are byte for byte what the exact filters (`SMI_BC1_NO_NBL`: nb5, `SMI_BC1_NO_NB5`: nb) and the oracle give -- on windows built to pass the line
filter by the fold alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DS = (-2, -1, 0, 1, 2)
BASE = {-2: 0, -1: 4, 0: 12, 1: 20, 2: 28}
MASK = {-2: 3, -1: 7, 0: 7, 1: 7, 2: 3}
M32 = np.uint64(0xFFFFFFFF)
U = np.uint64
LIST_SIZES = (1, 2, 2_000, 70_000)   # the last is above kN1MaxKeys (65,536): nb5 by the transposition, the others by atomics
BATCHES = (1, 12, 13, 64, 65, 1025)  # 5 n is / is not a multiple of 64 and of 256; 1025: more than one workgroup


def _lowmask(nbits):
    return U(0xFFFFFFFF) if nbits >= 32 else U((1 << nbits) - 1)


def n1_member(k, slot):
    """smi_bc.hip n1_member on a uint64 vector of 32-bit keys"""
    k = np.asarray(k, dtype=np.uint64)
    if slot < 48:
        return k ^ U((slot % 3 + 1) << (30 - 2 * (slot // 3)))
    if slot < 108:
        j = slot - 48
        sh = 30 - 2 * (1 + j // 4)
        return ((k & ~_lowmask(sh + 2)) | ((k & _lowmask(sh)) << U(2)) | U(j & 3)) & M32
    if slot < 168:
        j = slot - 108
        q = j // 4
        top = 32 - 2 * q
        return ((k & ~_lowmask(top) & M32) | U((j & 3) << (30 - 2 * q)) | ((k & _lowmask(top)) >> U(2))) & M32
    return k


def neighbourhood(keys):
    return np.unique(np.concatenate([n1_member(keys, s) for s in range(169)]))


def _core_flank(key, d):
    sh = 2 * (2 - d)
    core = (key >> U(sh)) & U(0xFFFFFF)
    low = U((1 << sh) - 1)
    return core, ((key >> U(24)) & ~low & U(0xFF)) | (key & low)


def nb5_cell(key, d):
    core, flank = _core_flank(key, d)
    return (core * U(40) + U((d + 2) * 8) + (flank >> U(5))) * U(32) + (flank & U(31))


def nbl_cell(key, d):
    core, flank = _core_flank(key, d)
    return ((core << U(5)) + U(BASE[d]) + ((flank >> U(5)) & U(MASK[d]))) * U(32) + (flank & U(31))


def _bits_digest(cells):
    """what k_bits_digest reports for a bitmap with exactly these bits set: count, sum of (word index mod 2^20) + 1 over the bits"""
    cells = np.unique(cells)
    return int(cells.size), int((((cells >> U(5)) & U(0xFFFFF)) + U(1)).sum())


def _key_list(synth, n):
    return synth.make_whitelist(max(n, 16), seed=171)[:n].numpy().astype(np.uint64)


def _bases16(x):
    return ((np.asarray(x, dtype=np.uint64)[:, None] >> (np.arange(15, -1, -1, dtype=np.uint64) * U(2))) & U(3)).astype(np.uint8)


def _records(stretch, five_prime, rng):
    """20-base stretches in KEY orientation (the key of key-side offset d is bases 2 - d .. 17 - d) -> (codes [n, 48], ae [n]) as the oracle and
    synth.pack_windows read them.  5': the record's bases 0 .. 19 are the stretch (key of offset o = bases 2 + o .., d = -o).  3': the key is the
    reverse complement of the record's bases 6 + o .., so bases 4 .. 23 are the stretch's reverse complement (d = o)."""
    n = stretch.shape[0]
    codes = rng.integers(0, 4, (n, 48), dtype=np.uint8)
    if five_prime:
        codes[:, 6:26] = stretch             # ae = 8: the 25-base record starts at 0-based index ae - 2
        ae = np.full(n, 8, dtype=np.int32)
    else:
        codes[:, 7 + 4:7 + 24] = 3 - stretch[:, ::-1]  # ae = 30: the 24-base record starts at 0-based index ae - 23
        ae = np.full(n, 30, dtype=np.int32)
    return codes, ae


def _stretches(keys_at, ds, rng):
    """random stretches with key keys_at[i] planted at key-side offset ds[i]"""
    s = rng.integers(0, 4, (keys_at.size, 20), dtype=np.uint8)
    b = _bases16(keys_at)
    for d in DS:
        sel = ds == d
        s[sel, 2 - d:18 - d] = b[sel]
    return s


def _stretch_keys(stretch, d):
    return (stretch[:, 2 - d:18 - d].astype(np.uint64) << (np.arange(15, -1, -1, dtype=np.uint64) * U(2))).sum(1)


def _window_set(keys, nbh, five_prime, seed, plant):
    """-> codes, ae, planted (indices of the fold-collision reads that no exact filter bit of any offset lets through)"""
    rng = np.random.default_rng(seed)
    sub = keys[rng.permutation(keys.size)[:50]]
    # every member of the subset's inverse one-step neighbourhood (the barcode and everything one mutation step away from it) at every offset
    members = np.concatenate([n1_member(sub, s) for s in range(169)])
    k_at = np.tile(members, 5)
    d_at = np.repeat(np.array(DS), members.size)
    planted = np.zeros(0, dtype=np.int64)
    if plant:
        # fold collisions: Z is in the neighbourhood, Y = Z with the one flank bit flipped that the fold drops (flank bit 7: the key's bit 31 at d = +2,
        # bit 7 at d = -2) is NOT -- Y's bit of nbl is set through Z, its bit of nb5 is clear
        z = members
        yk, yd = [], []
        for d, flip in ((2, 0x80000000), (-2, 0x80)):
            y = z ^ U(flip)
            y = y[~np.isin(y, nbh)]
            assert y.size > 100 and np.isin(nbl_cell(y, d), nbl_cell(nbh, d)).all() and not np.isin(nb5_cell(y, d), nb5_cell(nbh, d)).any()
            yk.append(y)
            yd.append(np.full(y.size, d))
        planted = k_at.size + np.arange(sum(y.size for y in yk))
        k_at = np.concatenate([k_at] + yk)
        d_at = np.concatenate([d_at] + yd)
    stretch = _stretches(k_at, d_at, rng)
    if plant:  # keep the planted reads whose five windows ALL miss the neighbourhood: the exact filters stop every probe, only the fold lets one through
        clean = np.ones(planted.size, dtype=bool)
        for d in DS:
            clean &= ~np.isin(_stretch_keys(stretch[planted], d), nbh)
        planted = planted[clean]
        assert planted.size > 150
    codes, ae = _records(stretch, five_prime, rng)
    # windows with N: in the core, in the flanks, at the base a deletion appends -- on copies of member reads and of planted ones
    n_src = np.concatenate([rng.integers(0, members.size * 5, 3000), planted[:200]]).astype(np.int64)
    nc = codes[n_src].copy()
    pos = rng.integers(5, 33, n_src.size)
    nc[np.arange(n_src.size), pos] = 4
    two = rng.random(n_src.size) < 0.3
    nc[two, rng.integers(5, 33, int(two.sum()))] = 4
    codes = np.concatenate([codes, nc])
    ae = np.concatenate([ae, ae[n_src]])
    ae[-20:] = 1  # windows that do not fit the read: found = -1, nothing looked up
    # a fixed shuffle, planted reads and N reads spread over the set (the small batches are its first reads), then some of each in front
    order = rng.permutation(codes.shape[0])
    front = np.concatenate([planted[:8] if plant else 2 + np.arange(8), [0, 1], k_at.size + np.arange(3)]).astype(np.int64)
    assert np.unique(front).size == 13
    order = np.concatenate([front, order[~np.isin(order, front)]])
    inv = np.empty_like(order)
    inv[order] = np.arange(order.size)
    return codes[order], ae[order], inv[planted]


def _run(pkg, ctx, d_win, n, five_prime):
    d_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    ctx.bc_match_device(d_win[:n].contiguous(), d_out, n, max_ed=1, five_prime=five_prime)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(pkg.BC_RESULT_DTYPE).reshape(-1)


@pytest.mark.parametrize("n", [500_000_000, 860_000_000])
def test_pair_index_width(pkg, synth, gpu_ctx, n):
    """the look-up kernel numbers its (read, offset) pairs in 32 bits where 5 n and the grid's stride fit them: 5 x 500 M passes 2^31 inside the 32-bit
    loop, 5 x 860 M passes 2^32 and takes the 64-bit one.  Blocks of real windows at the front, where the pair index passes 2^31, in the middle and at
    the end of a batch of empty records give what they give as a batch of their own; every other read comes out as an empty record does."""
    keys = _key_list(synth, 2_000)
    codes, ae, _ = _window_set(keys, neighbourhood(keys), False, seed=77, plant=True)
    block = synth.pack_windows(torch.from_numpy(codes[:256]), torch.from_numpy(ae[:256]), False).cuda()
    gpu_ctx.set_barcode_set(keys, mode=0)
    want = torch.zeros((256, 4), dtype=torch.int32, device="cuda")
    gpu_ctx.bc_match_device(block, want, 256, max_ed=1, five_prime=False)
    starts = [0, (1 << 31) // 5 - 100, n // 2, n - 256]
    d_win = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    for s in starts:
        d_win[s:s + 256] = block
    d_out = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    gpu_ctx.bc_match_device(d_win, d_out, n, max_ed=1, five_prime=False)
    torch.cuda.synchronize()
    assert int((want[:, 0] != 0).sum()) > 0 and want.view(torch.uint8).any()
    for s in starts:
        assert torch.equal(d_out[s:s + 256], want), s
    empty = d_out[300].clone()   # an empty record: found = -1
    assert int(d_out[300:301].cpu().numpy().view(pkg.BC_RESULT_DTYPE).reshape(-1)["found"][0]) == -1
    assert int((d_out != empty).any(dim=1).sum()) == int((want != empty).any(dim=1).sum()) * len(starts)
    del d_win, d_out
    torch.cuda.empty_cache()


def _oracle_found(st, exp):
    return np.where(st < 0, st, exp["found"])


@pytest.mark.parametrize("n_keys", LIST_SIZES)
def test_line_filter_table_and_records(pkg, synth, sor, gpu_ctx, monkeypatch, n_keys):
    keys = _key_list(synth, n_keys)
    small = n_keys <= 2_000
    nbh = neighbourhood(keys) if small else None
    sets = {}
    for five_prime in (False, True):
        codes, ae, planted = _window_set(keys, nbh, five_prime, seed=300 + n_keys % 97 + five_prime, plant=small)
        win = synth.pack_windows(torch.from_numpy(codes), torch.from_numpy(ae), five_prime).cuda()
        st, exp = sor.assign_batch(sor.BarcodeSet(keys), codes, ae, max_ed=1, five_prime=five_prime, n_threads=8)
        sets[five_prime] = (win, st, exp, planted, codes.shape[0])

    results, stats = {}, {}
    for cfg in ("default", "SMI_BC1_NO_NBL", "SMI_BC1_NO_NB5"):   # (the switches are read when a set is loaded)
        if cfg != "default":
            monkeypatch.setenv(cfg, "1")
        gpu_ctx.set_barcode_set(keys, mode=0)
        stats[cfg] = gpu_ctx.set_stats(digests=True)
        for five_prime, (win, _, _, _, n_all) in sets.items():
            for n in BATCHES + (n_all,):
                results[cfg, five_prime, n] = _run(pkg, gpu_ctx, win, n, five_prime)
        if cfg != "default":
            monkeypatch.delenv(cfg)
    gpu_ctx.set_barcode_set(keys, mode=0)  # leave the context with its filters on

    # the table
    a, b, c = stats["default"], stats["SMI_BC1_NO_NBL"], stats["SMI_BC1_NO_NB5"]
    assert a["nb5_bits"] == 5 * a["nb_bits"] == b["nb5_bits"] and a["nb5_digest"] == b["nb5_digest"]
    assert 0 < a["nbl_bits"] <= a["nb5_bits"]
    assert b["nbl_bits"] == b["nbl_digest"] == c["nbl_bits"] == c["nb5_bits"] == 0
    assert a["hbm_bytes"] - b["hbm_bytes"] == 1 << 31 and b["hbm_bytes"] - c["hbm_bytes"] == 5 << 29
    if small:
        assert (a["nb_bits"], a["nb5_bits"]) == (nbh.size, 5 * nbh.size)
        assert (a["nb5_bits"], a["nb5_digest"]) == _bits_digest(np.concatenate([nb5_cell(nbh, d) for d in DS]))
        assert (a["nbl_bits"], a["nbl_digest"]) == _bits_digest(np.concatenate([nbl_cell(nbh, d) for d in DS]))

    # the records
    for five_prime, (win, st, exp, planted, n_all) in sets.items():
        exp_found = _oracle_found(st, exp)
        for n in BATCHES + (n_all,):
            got = results["default", five_prime, n]
            for cfg in ("SMI_BC1_NO_NBL", "SMI_BC1_NO_NB5"):
                assert (got.view(np.uint8) == results[cfg, five_prime, n].view(np.uint8)).all(), (cfg, five_prime, n)
            assert (got["found"] == exp_found[:n]).all(), (five_prime, n)
            sel = exp_found[:n] == 1
            for f in ("bc", "ed", "ed_sec", "offset", "ins_minus_del"):
                e = exp[f][:n][sel].astype(np.int64) & (0xFFFFFFFF if f == "bc" else -1)
                assert (got[f][sel].astype(np.int64) == e).all(), (f, five_prime, n)
            assert (got["n_matches"][st[:n] >= 0] == exp["n_matches"][:n][st[:n] >= 0]).all(), (five_prime, n)
        full = results["default", five_prime, n_all]
        assert int((full["found"] == 1).sum()) > 1000 * min(n_keys, 50) // 50 + 100
        if planted.size:  # passed the line filter by the fold alone: looked up, no entry, not found and no match counted
            assert (full["found"][planted] == 0).all() and (full["n_matches"][planted] == 0).all()
