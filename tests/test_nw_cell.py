"""The Needleman-Wunsch cell of csrc/smi_nw.h in six VALU operations against the seven-operation cell it replaces (kept as -DSMI_NW_CELL7=1),
in plain Python and without a GPU.

Both integer cells are restated here as the header writes them -- the packed value, the constants added to the three predecessors, the
two-operand maxima at the band's edges, nw_errors' counter and lead fields under the shift -- over a batch of match matrices at a time
(numpy only carries the batch; every operation is the kernel's integer operation).  The two must agree on the move tag of EVERY cell of the
band, on the corner score and on nw_errors' (#x, lead); and the alignment strings traced from the new tags must be the ones of the
reference's full fill (pymodel_scan.needleman) on the gate-passing slices test_nw_band builds.
"""
import random

import numpy as np
import pytest

from pymodel_scan import ENC4, needleman
from test_nw_band import PATTERNS, n_kmers_matching, nw_band, slices_for

SH = 11                      # nw_errors: the tagged score sits above q (6 bits at 5) and lead (5 bits at 0)
BIAS = -(1 << 20)            # the new cell's row 0 (a multiple of 4: it reaches neither the tag nor a comparison)
BIAS_E = -(1 << 16)          # ... and nw_errors', under << SH
I32 = 1 << 31


def _band(r, n, w):
    return max(1, r - w), min(n, r + w)


def _const(b, v):
    return np.full(b, v, dtype=np.int64)


def _in_range(v):
    assert (v >= -I32).all() and (v < I32).all()  # the kernels compute in 32-bit registers
    return v


# ---- the parent's cell: U = 4 * score + 2 + 20 * r, tags 3 match / 2 mismatch / 1 up / 0 left --------------------------------------------
def fill7(M, w):
    """M: bool [B, N, N], M[:, r - 1, c - 1] = read base r matches pattern base c -> (tags [B, N + 1, N + 1], -1 outside the band; corner score)"""
    b, n = M.shape[0], M.shape[1]
    U = [_const(b, -20 * c + 2) for c in range(n + 1)]
    tags = np.full((b, n + 1, n + 1), -1, dtype=np.int8)
    for r in range(1, n + 1):
        clo, chi = _band(r, n, w)
        diag = U[clo - 1]
        if r <= w:
            U[0] = _const(b, 4 * r + 2)
        for c in range(clo, chi + 1):
            d = diag + 41 * M[:, r - 1, c - 1]
            if c - r == w:
                v = np.maximum(d, U[c - 1] - 22)
            elif r - c == w:
                v = np.maximum(d, U[c] - 1)
            else:
                v = np.maximum(np.maximum(d, U[c] - 1), U[c - 1] - 22)
            diag = U[c]
            U[c] = (_in_range(v) & ~3) | 2
            tags[:, r, c] = v & 3
    assert ((U[n] - 2 - 20 * n) % 4 == 0).all()
    return tags, (U[n] - 2 - 20 * n) // 4


def errors7(M, w):
    """-> (#x, lead) of the parent's nw_errors: cell = (4 * score + 2 + 20 r) << 11 | q << 5 | lead, q = 32 + #up - #match"""
    b, n = M.shape[0], M.shape[1]
    kmatch = (41 << SH) - 32
    U = [_const(b, ((-20 * c + 2) << SH) + (32 << 5)) for c in range(n + 1)]
    for r in range(1, n + 1):
        clo, chi = _band(r, n, w)
        diag = U[clo - 1]
        if r <= w:
            U[0] = _const(b, ((4 * r + 2) << SH) + ((32 + r) << 5) + r)
        for c in range(clo, chi + 1):
            d = diag + kmatch * M[:, r - 1, c - 1]
            if c - r == w:
                v = np.maximum(d, U[c - 1] - (22 << SH))
            elif r - c == w:
                v = np.maximum(d, U[c] - (1 << SH) + 32)
            else:
                v = np.maximum(np.maximum(d, U[c] - (1 << SH) + 32), U[c - 1] - (22 << SH))
            diag = U[c]
            U[c] = (_in_range(v) & ~(3 << SH)) | (2 << SH)
    return n + ((U[n] >> 5) & 63) - 32, U[n] & 31


# ---- the new cell: T = 4 * score + 36 * r + 20 * c (+ bias), tags 3 mismatch / 2 match / 1 up / 0 left -----------------------------------
def fill6(M, w):
    b, n = M.shape[0], M.shape[1]
    T = [_const(b, BIAS) for _ in range(n + 1)]          # row 0: 4 * (-5 c) + 20 c = 0
    tags = np.full((b, n + 1, n + 1), -1, dtype=np.int8)
    for r in range(1, n + 1):
        clo, chi = _band(r, n, w)
        diag = T[clo - 1]
        if r <= w:
            T[0] = _const(b, BIAS + 20 * r)              # column 0: 4 * (-4 r) + 36 r
        for c in range(clo, chi + 1):
            d = (39 << M[:, r - 1, c - 1].astype(np.int64)) + diag   # v_lshl_add_u32: mismatch + 39, match + 78
            if c - r == w:
                v = np.maximum(d, T[c - 1])
            elif r - c == w:
                v = np.maximum(d, T[c] + 17)
            else:
                v = np.maximum(np.maximum(d, T[c] + 17), T[c - 1])
            diag = T[c]
            T[c] = _in_range(v) & ~3
            tags[:, r, c] = v & 3
    assert ((T[n] - BIAS - 56 * n) % 4 == 0).all()
    return tags, (T[n] - BIAS - 56 * n) // 4


def errors6(M, w):
    """-> (#x, lead) of the new nw_errors: q starts at 2 N, a mismatch takes 1 off it and a match 2, so that it ends as #x itself"""
    b, n = M.shape[0], M.shape[1]
    assert 2 * n <= 63
    kmatch = (39 << SH) - 32
    bias = BIAS_E * (1 << SH)
    T = [_const(b, bias + ((2 * n) << 5)) for _ in range(n + 1)]
    for r in range(1, n + 1):
        clo, chi = _band(r, n, w)
        diag = T[clo - 1]
        if r <= w:
            T[0] = _const(b, bias + ((20 * r) << SH) + ((2 * n) << 5) + r)
        for c in range(clo, chi + 1):
            d = (kmatch << M[:, r - 1, c - 1].astype(np.int64)) + diag
            if c - r == w:
                v = np.maximum(d, T[c - 1])
            elif r - c == w:
                v = np.maximum(d, T[c] + (17 << SH))
            else:
                v = np.maximum(np.maximum(d, T[c] + (17 << SH)), T[c - 1])
            diag = T[c]
            T[c] = _in_range(v) & ~(3 << SH)
            assert (((T[c] >> 5) & 63) >= 2 * n - 2 * min(r, c)).all()   # no partial path borrows from the tag
    return (T[n] >> 5) & 63, T[n] & 31


SWAP = np.array([0, 1, 3, 2, -1], dtype=np.int8)   # new tag -> the parent's code (match and mismatch trade places); -1 stays -1


def _assert_equal_cells(M, w):
    t7, s7 = fill7(M, w)
    t6, s6 = fill6(M, w)
    assert (SWAP[t6] == t7).all()                  # every cell of the band, not only the path
    assert (s6 == s7).all()
    n = M.shape[1]
    if n <= 27:
        x7, l7 = errors7(M, w)
        x6, l6 = errors6(M, w)
        assert (x6 == x7).all() and (l6 == l7).all()
        return t6, x6, l6
    return t6, None, None


@pytest.mark.parametrize("w", [1, 2, 4])
def test_all_4x4_matrices(w):
    bits = np.arange(1 << 16, dtype=np.int64)
    M = ((bits[:, None] >> np.arange(16)[None, :]) & 1).astype(bool).reshape(-1, 4, 4)
    _assert_equal_cells(M, w)


RANDOM_CASES = [(10, 3), (16, 7), (22, 12), (22, nw_band(22, 6)), (25, nw_band(25, 5)), (25, nw_band(25, 6)), (27, nw_band(27, 5)),
                (27, nw_band(27, 6)), (10, 10), (16, 16), (27, 27)]


@pytest.mark.parametrize("n,w", RANDOM_CASES)
@pytest.mark.parametrize("density", [0.25, 0.5, 0.9])
def test_random_matrices(n, w, density):
    """the diagonal matches with probability `density`, every other cell with 1/4 (a random base): paths with ties, gaps and runs"""
    assert (nw_band(10, 5), nw_band(16, 5), nw_band(22, 5)) == (3, 7, 12)
    rng = np.random.default_rng(7000 + 100 * n + w + int(100 * density))
    b = 3000
    M = rng.random((b, n, n)) < 0.25
    idx = np.arange(n)
    M[:, idx, idx] = rng.random((b, n)) < density
    t6, nx, lead = _assert_equal_cells(M, w)
    if w == n:   # the full matrix: nw_errors' two fields are what the walk over nw_full's tags counts (a band may cut the walk's cells off)
        for k in range(0, b, 50):
            wx, wl = _walk_counts(t6[k], n)
            assert (wx, wl) == (int(nx[k]), int(lead[k]))


def _walk(tags, n):
    """the path from (N, N) to (0, 0) by the new tags -> the moves in walk order ('m' match, 's' mismatch, 'u' up, 'l' left)"""
    r = c = n
    out = []
    while r > 0 or c > 0:
        if r == 0:
            t = 0
        elif c == 0:
            t = 1
        else:
            t = int(tags[r][c])
            assert t >= 0, "the walk left the band"
        out.append("lums"[t])
        if t >= 2:
            r, c = r - 1, c - 1
        elif t == 1:
            r -= 1
        else:
            c -= 1
    return out


def _walk_counts(tags, n):
    moves = _walk(tags, n)
    lead = 0
    while lead < len(moves) and moves[len(moves) - 1 - lead] == "u":
        lead += 1
    return sum(m != "m" for m in moves), lead


def _strings(tags, pat_s, sl_s):
    """(tmpl, dots, read) as SequenceAlignment.getTraceback writes them, from the tags"""
    n = len(pat_s)
    r = c = n
    tmpl, dots, read = [], [], []
    for m in _walk(tags, n):
        tmpl.append(pat_s[c - 1] if m != "u" else "-")
        read.append(sl_s[r - 1] if m != "l" else "-")
        dots.append("." if m == "m" else "x")
        if m in "ms":
            assert ((ENC4[pat_s[c - 1]] & ENC4[sl_s[r - 1]]) != 0) == (m == "m")   # tag 2 is a match, tag 3 a mismatch
            r, c = r - 1, c - 1
        elif m == "u":
            r -= 1
        else:
            c -= 1
    return "".join(reversed(tmpl)), "".join(reversed(dots)), "".join(reversed(read))


@pytest.mark.parametrize("n,min_kmers,min_diag", [(10, 2, 5), (16, 2, 5), (22, 2, 5), (27, 2, 5), (22, 3, 6)])
def test_traced_alignment_is_the_reference_s(n, min_kmers, min_diag):
    rng = random.Random(2000 + 7 * n + min_kmers)
    pat_s = PATTERNS[n]
    pat = [ENC4[ch] for ch in pat_s]
    w = nw_band(n, min_diag)
    kept = []
    for s in slices_for(pat_s, rng, 500 if n <= 16 else 300):
        if n_kmers_matching(pat, [ENC4[ch] for ch in s]) >= min_kmers:   # the kernels align nothing else
            kept.append(s)
    assert len(kept) > 100
    codes = np.array([[ENC4[ch] for ch in s] for s in kept], dtype=np.int64)
    M = (codes[:, :, None] & np.array(pat, dtype=np.int64)[None, None, :]) != 0
    t6, nx, lead = _assert_equal_cells(M, w)
    for k, s in enumerate(kept):
        ref = needleman(pat, [ENC4[ch] for ch in s])
        assert _strings(t6[k], pat_s, s) == ref, s
        if n <= 27:   # nw_errors' fields are the strings' own counts
            assert int(nx[k]) == ref[1].count("x") and int(lead[k]) == len(ref[0]) - len(ref[0].lstrip("-")), s
