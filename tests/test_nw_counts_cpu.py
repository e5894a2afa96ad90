"""nw_counts of csrc/smi_nw.h -- the Needleman-Wunsch cell that carries (#x, up, trail, lead) below its tagged score, which K-SCAN's TSO round runs
in place of the fill with tags and the walk -- in plain Python and without a GPU.

The cell is restated here as the header writes it: the packed value with its exact field layout and bias, the constants added to the three
predecessors, the two-operand maxima at the band's edges, the extra add of row N (numpy only carries the batch; every operation is the kernel's
32-bit integer operation).  Beside the packed value the model carries every field as a number of its own, handed on by the tag of the maximum: a field
that left its width, borrowed from or carried into a neighbour shows as a difference between the two.  (#x, lead, up, trail) and what the kernel makes
of them (ne, nmis, ins, del) are compared with the walk over nw_full's tags (tests/test_nw_cell.py fill6) and, on slices of bases, with the oracle's
sor_nw_stats.
"""
import ctypes
import random

import numpy as np
import pytest

from pymodel_scan import ENC4
from test_nw_band import PATTERNS, n_kmers_matching, nw_band, slices_for
from test_nw_cell import _walk, fill6

N, W = 16, 7
LEAD_BITS, TRAIL_BITS, UP_BITS, Q_BITS = 3, 3, 5, 6          # from the bottom: lead, trail, up, q; then the 2 tag bits and the score
TRAIL_POS = LEAD_BITS
UP_POS = TRAIL_POS + TRAIL_BITS
Q_POS = UP_POS + UP_BITS
SH = Q_POS + Q_BITS                                          # 17: 19 bits below the score, 13 signed bits for it
BIAS = -(1 << (12 + SH))
I32 = 1 << 31
TSO = PATTERNS[16]


class FieldOverflow(AssertionError):
    pass


ALL_FIELDS = ("q", "up", "trail", "lead")


def counts6(M, w, widths=ALL_FIELDS, packed=True):
    """M: bool [B, n, n], M[:, r - 1, c - 1] = read base r matches pattern base c -> dict of (#x, lead, up, trail) arrays, read off the packed corner cell,
    and "widest": the largest value each field took in any cell.
    widths: the fields checked against their width in every cell (FieldOverflow); packed: the packed fields are checked against the model's own counts"""
    b, n = M.shape[0], M.shape[1]
    kmatch = (39 << SH) - (1 << Q_POS)
    k_up = (17 << SH) + (1 << UP_POS)
    k_trail = 1 << TRAIL_POS

    def const(v):
        return np.full(b, v, dtype=np.int64)

    U = [const(BIAS + ((2 * n) << Q_POS)) for _ in range(n + 1)]
    # the fields as numbers of their own: (q, up, trail, lead) per column
    F = [np.stack([const(2 * n), const(0), const(0), const(0)]) for _ in range(n + 1)]
    widest = dict.fromkeys(ALL_FIELDS, 0)
    for r in range(1, n + 1):
        clo, chi = max(1, r - w), min(n, r + w)
        diag, fdiag = U[clo - 1], F[clo - 1]
        if r <= w:
            U[0] = const(BIAS + ((20 * r) << SH) + ((2 * n) << Q_POS) + (r << UP_POS) + r)
            F[0] = np.stack([const(2 * n), const(r), const(0), const(r)])
            _check(U[0], F[0], r, 0, n, widths, packed, widest)
        for c in range(clo, chi + 1):
            m = M[:, r - 1, c - 1].astype(np.int64)
            d = (kmatch << m) + diag                               # v_lshl_add_u32
            left = U[c - 1] + k_trail if r == n else U[c - 1]
            up = U[c] + k_up
            if c - r == w:
                v = np.maximum(d, left)
            elif r - c == w:
                v = np.maximum(d, up)
            else:
                v = np.maximum(np.maximum(d, up), left)
            assert (v >= -I32).all() and (v < I32).all() and (v < 0).all()   # 32-bit registers; the bias keeps every cell negative
            tag = (v >> SH) & 3
            # the fields of the predecessor the tag names, moved as the constants move them
            fd = fdiag - np.stack([1 + m, 0 * m, 0 * m, 0 * m])
            fu = F[c] + np.stack([0 * m, 1 + 0 * m, 0 * m, 0 * m])
            fl = F[c - 1] + np.stack([0 * m, 0 * m, (1 if r == n else 0) + 0 * m, 0 * m])
            f = np.where(tag >= 2, fd, np.where(tag == 1, fu, fl))
            diag, fdiag = U[c], F[c]
            U[c] = v & ~(3 << SH)
            F[c] = f
            _check(U[c], f, r, c, n, widths, packed, widest)
    u = U[n]
    return dict(nx=(u >> Q_POS) & ((1 << Q_BITS) - 1), lead=u & ((1 << LEAD_BITS) - 1), up=(u >> UP_POS) & ((1 << UP_BITS) - 1),
                trail=(u >> TRAIL_POS) & ((1 << TRAIL_BITS) - 1), widest=widest)


def _check(u, f, r, c, n, widths, packed, widest):
    q, up, trail, lead = f
    for name, val, bits in (("q", q, Q_BITS), ("up", up, UP_BITS), ("trail", trail, TRAIL_BITS), ("lead", lead, LEAD_BITS)):
        widest[name] = max(widest[name], int(val.max()))
        if name in widths and not ((val >= 0).all() and (val < (1 << bits)).all()):
            raise FieldOverflow("%s = %d at (%d, %d)" % (name, int(val.max()), r, c))
    assert (q >= 2 * n - 2 * min(r, c)).all() and (up <= r).all()      # the header's argument: no borrow from the tag, no carry out of up
    if packed:
        assert (((u >> Q_POS) & 63) == q).all() and (((u >> UP_POS) & 31) == up).all() and (((u >> TRAIL_POS) & 7) == trail).all() and ((u & 7) == lead).all()
    assert ((u >> SH) & 3 == 0).all()


def walk_counts(tags, n):
    """(#x, lead, up, trail) and (ne, nmis, ins, del) as nw_walk_bits reads them off the step masks"""
    mv = _walk(tags, n)
    lead = 0
    while lead < len(mv) and mv[len(mv) - 1 - lead] == "u":
        lead += 1
    trail = 0
    while trail < len(mv) and mv[trail] == "l":
        trail += 1
    nx, up, left, sub = sum(m != "m" for m in mv), mv.count("u"), mv.count("l"), mv.count("s")
    assert up == left
    return (nx, lead, up, trail), derived(nx, lead, up, trail, d=left, sub=sub)


def derived(nx, lead, up, trail, d=None, sub=None):
    """the caller's arithmetic (smi_scan.hip); with d and sub: the walk's own sums"""
    ne = np.float32(nx) - np.float32(0.9) * np.float32(lead)           # two roundings
    if d is None:
        dl = int(np.int8(up - trail))
        return float(ne), nx - trail, up, dl
    dl = int(np.int8(d - trail))
    return float(ne), up + dl + sub, up, dl


def gated(M):
    """> 1 matching 4-mers on the main diagonal (Kmers.nKmersMatching_4mer)"""
    n = M.shape[1]
    dg = M[:, np.arange(n), np.arange(n)]
    k = dg[:, :-3] & dg[:, 1:-2] & dg[:, 2:-1] & dg[:, 3:]
    return k.sum(1) > 1


def _assert_counts_equal_walk(M, w=W, every=1):
    got = counts6(M, w)
    tags, _ = fill6(M, w)
    n = M.shape[1]
    out = []
    for k in range(0, M.shape[0], every):
        raw, der = walk_counts(tags[k], n)
        mine = (int(got["nx"][k]), int(got["lead"][k]), int(got["up"][k]), int(got["trail"][k]))
        assert mine == raw, k
        assert derived(*mine) == der, k
        out.append(raw)
    return out


def test_layout():
    assert nw_band(16, 5) == W and SH == 17 and SH + 2 + 13 == 32
    assert W < (1 << LEAD_BITS) and W < (1 << TRAIL_BITS) and N < (1 << UP_BITS) and 2 * N < (1 << Q_BITS)
    assert 56 * N + 78 < (1 << 12)                                      # 4*score + 36 r + 20 c (+ the diagonal's constant) against the bias


def random_gated(rng, b, density):
    """the diagonal matches with probability `density`, every other cell with 1/4 (a random base), and five matches in a row planted on the diagonal:
    what the 4-mer gate guarantees, and no more of it at a low density"""
    M = rng.random((b, N, N)) < 0.25
    idx = np.arange(N)
    M[:, idx, idx] = rng.random((b, N)) < density
    p = rng.integers(0, N - 4, size=b)
    for j in range(5):
        M[np.arange(b), p + j, p + j] = True
    assert gated(M).all()
    return M


@pytest.mark.parametrize("density", [0.1, 0.3, 0.5, 0.7, 0.9])
def test_random_gated_matrices(density):
    M = random_gated(np.random.default_rng(9100 + int(100 * density)), 1000, density)
    raws = _assert_counts_equal_walk(M)
    assert len({r[2] for r in raws}) >= 3 and any(r[1] for r in raws) and any(r[3] for r in raws)   # gaps, leading and trailing ones among them


def test_ties_are_decided_by_the_tag():
    """cells ON the path at which two or three predecessors tie in score: the counts follow the predecessor the tag order names (diag >= up >= left)"""
    M = random_gated(np.random.default_rng(9200), 2500, 0.5)
    # scores of the full band by the plain recurrence
    b = M.shape[0]
    NEG = -10 ** 6
    S = np.full((b, N + 1, N + 1), NEG, dtype=np.int64)
    S[:, 0, :W + 1] = -5 * np.arange(W + 1)
    S[:, :W + 1, 0] = -4 * np.arange(W + 1)
    tie = np.zeros((b, N + 1, N + 1), dtype=np.int8)                    # 1 diag = up, 2 diag = left, 4 up = left (among the maxima)
    for r in range(1, N + 1):
        for c in range(max(1, r - W), min(N, r + W) + 1):
            d = S[:, r - 1, c - 1] + np.where(M[:, r - 1, c - 1], 5, -5)
            u = S[:, r - 1, c] - 5 if c - r < W else np.full(b, NEG)
            l = S[:, r, c - 1] - 5 if r - c < W else np.full(b, NEG)
            best = np.maximum(np.maximum(d, u), l)
            S[:, r, c] = best
            tie[:, r, c] = ((d == best) & (u == best)) * 1 + ((d == best) & (l == best)) * 2 + ((u == best) & (l == best)) * 4
    tags, _ = fill6(M, W)
    got = counts6(M, W)
    seen = [0, 0, 0]
    for k in range(b):
        r = c = N
        on_path = 0
        for m in _walk(tags[k], N):
            if r > 0 and c > 0:
                on_path |= int(tie[k, r, c])
            if m in "ms":
                r, c = r - 1, c - 1
            elif m == "u":
                r -= 1
            else:
                c -= 1
        if on_path:
            raw, _ = walk_counts(tags[k], N)
            assert (int(got["nx"][k]), int(got["lead"][k]), int(got["up"][k]), int(got["trail"][k])) == raw
            for j in range(3):
                seen[j] += (on_path >> j) & 1
    assert min(seen) > 20, seen


# ---- structured cases -------------------------------------------------------------------------------------------------------------------------
def _eye(shift_rows=0):
    """read base r matches pattern base c iff r - c == shift_rows"""
    M = np.zeros((N, N), dtype=bool)
    for c in range(N):
        if 0 <= c + shift_rows < N:
            M[c + shift_rows, c] = True
    return M


def _from(read_of_col):
    """match matrix of a read whose base r is a copy of pattern base read_of_col[r] (-1: a base that matches nothing)"""
    M = np.zeros((N, N), dtype=bool)
    for r, c in enumerate(read_of_col):
        if c >= 0:
            M[r, c] = True
    return M


def _one(M):
    raw = _assert_counts_equal_walk(M[None], W)[0]
    return dict(zip(("nx", "lead", "up", "trail"), raw))


def test_all_matches():
    assert _one(_eye()) == dict(nx=0, lead=0, up=0, trail=0)
    assert _one(np.ones((N, N), dtype=bool)) == dict(nx=0, lead=0, up=0, trail=0)


def test_all_mismatches_on_a_gated_slice():
    M = np.zeros((N, N), dtype=bool)
    M[np.arange(5), np.arange(5)] = True               # five matches on the diagonal, as the gate guarantees, and nothing else
    assert gated(M[None])[0]
    assert _one(M) == dict(nx=11, lead=0, up=0, trail=0)
    assert _one(np.zeros((N, N), dtype=bool))["up"] == 0   # (not gated: the two fills still agree on the band)


@pytest.mark.parametrize("k", range(1, 8))
def test_leading_template_gaps_and_trailing_read_gaps_together(k):
    """the read is k bases of nothing and then the pattern: k up moves in column 0, the diagonal, k left moves that end the path in row N"""
    got = _one(_eye(k))
    assert got == dict(nx=2 * k, lead=k, up=k, trail=k)
    ne, nmis, ins, dl = derived(**got)
    assert (nmis, ins, dl) == (k, k, 0) and abs(ne - (2 * k - 0.9 * k)) < 1e-5


@pytest.mark.parametrize("k", range(1, 8))
def test_leading_template_gaps(k):
    """k bases of nothing, the pattern's start, and k pattern bases missing in the interior: lead = k, no trailing read gap, del = k"""
    a = (N - k) // 2
    cols = [-1] * k + list(range(a)) + list(range(a + k, N))
    got = _one(_from(cols))
    assert got == dict(nx=2 * k, lead=k, up=k, trail=0)
    assert derived(**got)[1:] == (2 * k, k, k)


@pytest.mark.parametrize("k", range(1, 8))
def test_trailing_read_gaps(k):
    """k bases of nothing inserted in the interior push the pattern's last k bases off the read: up moves in the interior, trail = k, del = 0 != ins"""
    a = (N - k) // 2
    cols = list(range(a)) + [-1] * k + list(range(a, N - k))
    got = _one(_from(cols))
    assert got == dict(nx=2 * k, lead=0, up=k, trail=k)
    assert derived(**got)[1:] == (k, k, 0)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_up_run_and_left_run_in_the_interior(k):
    cols = list(range(4)) + [-1] * k + list(range(4, 9)) + list(range(9 + k, N))
    got = _one(_from(cols))
    assert got == dict(nx=2 * k, lead=0, up=k, trail=0)
    assert derived(**got)[1:] == (2 * k, k, k)


def test_path_along_the_band_s_edges():
    """W = 7 gaps at once: the path runs down the band's lower edge (r - c = 7) and, with the gaps the other way round, along its upper edge"""
    low = _one(_eye(7))
    assert low["lead"] == 7 and low["trail"] == 7
    # the pattern's first seven bases missing at the read's start cannot be had (leading read gaps are left moves of row 0, then the diagonal c - r = 7)
    M = np.zeros((N, N), dtype=bool)
    for r in range(N - 7):
        M[r, r + 7] = True
    up = _one(M)
    assert up == dict(nx=14, lead=0, up=7, trail=0)     # seven read gaps first, the diagonal on the edge, seven up moves that end the path


def test_widths_hold_where_the_header_asserts_them_and_not_beyond():
    """Over the band every field stays inside its width (counts6 checks each cell of every test above).  The full matrix shows where the static_asserts
    must sit: `up` reaches N = 16 and still fits its five bits, `lead` reaches 8 in row 8 and does not fit three -- lead and trail rest on W < 8, not on N."""
    rng = np.random.default_rng(9300)
    M = rng.random((500, N, N)) < 0.25
    w = counts6(M, W)["widest"]                         # any matrix, gated or not: the widths are a property of the band
    assert w["lead"] <= W and w["trail"] <= W and w["up"] <= N and w["q"] == 2 * N
    nothing = np.zeros((1, N, N), dtype=bool)           # nothing matches: column 0 of the full matrix carries lead = up = r up to 16
    with pytest.raises(FieldOverflow, match=r"lead = 8 at \(8, 0\)"):
        counts6(nothing, N)
    # up forced to its widest: the full matrix with lead and trail left unchecked (they ran into their neighbours, so the packed word is not compared)
    w = counts6(nothing, N, widths=("q", "up"), packed=False)["widest"]
    assert w["up"] == N < (1 << UP_BITS) and w["lead"] == N >= (1 << LEAD_BITS)
    # a path with N left moves in row N: all matches in the first row only -- trail would need five bits without the band
    top = np.zeros((1, N, N), dtype=bool)
    w = counts6(top, N, widths=("q", "up"), packed=False)["widest"]
    assert w["trail"] <= N


# ---- against the oracle -----------------------------------------------------------------------------------------------------------------------
def _oracle(sor, sl):
    L = sor.lib()
    L.sor_nw_stats.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    o9, f2 = np.zeros(9, dtype=np.int32), np.zeros(2, dtype=np.float32)
    assert L.sor_nw_stats(TSO.encode(), sl.encode(), o9.ctypes.data, f2.ctypes.data, None) == 0
    return float(f2[0]), int(o9[2]), int(o9[5]), int(o9[4])              # ne, nmis, ins, del


def _matrix(slices):
    pat = np.array([ENC4[ch] for ch in TSO], dtype=np.int64)
    codes = np.array([[ENC4[ch] for ch in s] for s in slices], dtype=np.int64)
    return (codes[:, :, None] & pat[None, None, :]) != 0


def test_against_the_oracle_on_gated_slices(sor):
    rng = random.Random(9400)
    pat = [ENC4[ch] for ch in TSO]
    kept = [s for s in slices_for(TSO, rng, 3000) if n_kmers_matching(pat, [ENC4[ch] for ch in s]) >= 2]
    # the structured shapes in bases, where bases can say them and the slice passes the gate: a long enough stretch of the pattern stays on the diagonal
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    for k in range(1, 8):
        junk = "".join(comp[ch] for ch in TSO[8:8 + k])
        kept.append(TSO[:8] + junk + TSO[8:16 - k])          # an insertion behind eight bases: up moves, trailing read gaps
        kept.append((TSO[:8] + TSO[8 + k:] + "C" * k)[:16])  # a deletion behind eight bases
        kept.append(junk + TSO[:16 - k])                     # leading template gaps (gated only where the shifted pattern happens to be)
    kept = [s for s in kept if len(s) == 16 and n_kmers_matching(pat, [ENC4[ch] for ch in s]) >= 2]
    assert len(kept) > 1500
    got = counts6(_matrix(kept), W)
    n_del_ne_ins = 0
    for k, s in enumerate(kept):
        mine = derived(int(got["nx"][k]), int(got["lead"][k]), int(got["up"][k]), int(got["trail"][k]))
        ref = _oracle(sor, s)
        assert mine == ref, (s, mine, ref)
        n_del_ne_ins += mine[2] != mine[3]
    assert n_del_ne_ins > 50
