"""Cases of tests/test_poa_edges_cpu.py and tests/test_poa_edges_gpu.py (test infrastructure only): molecules that put K-POA and the model
on the edges of their loops -- read lengths and gap ends on the 64-column chunk seams, gaps longer than one base in the read (the E carry)
and in the graph (the F states), both gap types and their tie at L = 2, ties of the end cell, wide aligned groups, many reads, and int16 rows
at the top of their range.  Next to them a second reference: `literal_align`, DESIGN.md section 8c's rules 1 and 3-6 written cell by cell
from the rule text in plain Python ints (E opened from H, no prefix maximum, its own traceback), `path_score`, which re-scores a traceback
under rule 1, and mutant switches on the literal that show which case notices which mistake.  Everything comes from fixed seeds."""
import functools
import zlib

import numpy as np

import consensusmodel as cm

MATCH, MISMATCH, G, E, Q, C = 5, -4, -8, -6, -10, -4      # rule 1, typed again here on purpose
NEG = -10 ** 9
CHUNK = 64                                                # K-POA's columns per step


def gap_score(length, one_gap_type=False):
    """rule 1: a gap of length L scores max(g + (L-1) e, q + (L-1) c)"""
    a = G + (length - 1) * E
    return a if one_gap_type else max(a, Q + (length - 1) * C)


# ---- the literal reference --------------------------------------------------------------------------------------------------------------
def literal_align(graph, read, chunk_carry=True, one_gap_type=False, f2_first=False, last_max=False, high_rank=False, no_ring=False, out=None):
    """rules 1 and 3-6, one cell at a time.  Rows are lists indexed by the read position j = 0 .. n (column 0: H = 0, E = -inf); a node
    without predecessors takes the virtual row (H = 0, F = -inf).  E1 / E2 are running recurrences opened from H.  The keywords are the
    mutants (no_ring acts in literal_poa)."""
    n, N = len(read), len(graph.base)
    aln = [-1] * n
    if out is not None:
        out["best"] = 0
    if n == 0 or N == 0:
        return aln
    order = graph.topo()                                   # rule 3 (cm.Graph)
    rank = {v: i for i, v in enumerate(order)}
    preds = {v: graph.preds(v) for v in order}
    H, F1, F2, E1, E2 = {}, {}, {}, {}, {}
    best, bv, bj = 0, -1, -1
    for v in order:
        ps = preds[v]
        h, f1, f2, e1, e2 = [0] * (n + 1), [NEG] * (n + 1), [NEG] * (n + 1), [NEG] * (n + 1), [NEG] * (n + 1)
        for j in range(1, n + 1):
            s = MATCH if read[j - 1] == graph.base[v] else MISMATCH
            if ps:
                m = max(H[p][j - 1] for p in ps) + s
                f1[j] = max(max(H[p][j] + G, F1[p][j] + E) for p in ps)
                f2[j] = max(max(H[p][j] + Q, F2[p][j] + C) for p in ps)
            else:
                m = 0 + s
                f1[j] = 0 + G
                f2[j] = 0 + Q
            e1[j] = max(h[j - 1] + G, e1[j - 1] + E)
            e2[j] = max(h[j - 1] + Q, e2[j - 1] + C)
            if not chunk_carry and j > 1 and (j - 1) % CHUNK == 0:      # mutant: nothing comes in from the columns of the last chunk
                e1[j] = e2[j] = NEG
            if one_gap_type:
                f2[j] = e2[j] = NEG
            h[j] = max(0, m, f1[j], f2[j], e1[j], e2[j])
            if h[j] > best or (last_max and h[j] == best and best > 0):  # rule 5
                best, bv, bj = h[j], v, j
        H[v], F1[v], F2[v], E1[v], E2[v] = h, f1, f2, e1, e2
    if out is not None:
        out["best"] = best
    if best <= 0:
        return aln
    pick = (lambda c: max(c, key=rank.get)) if high_rank else (lambda c: min(c, key=rank.get))
    states = ("F2", "F1", "E2", "E1") if f2_first else ("F1", "F2", "E1", "E2")
    rows = {"F1": (F1, G, E), "F2": (F2, Q, C), "E1": (E1, G, E), "E2": (E2, Q, C)}
    v, j, state = bv, bj, "H"
    while True:                                            # rule 6
        if state == "H":
            h = H[v][j]
            if h == 0:
                break
            s = MATCH if read[j - 1] == graph.base[v] else MISMATCH
            ps = preds[v]
            m = (max(H[p][j - 1] for p in ps) if ps else 0) + s
            if h == m:
                aln[j - 1] = v
                if not ps or j == 1:
                    break
                v, j = pick([p for p in ps if H[p][j - 1] + s == m]), j - 1
            else:
                state = next(st for st in states if rows[st][0][v][j] == h)
        elif state in ("F1", "F2"):
            Fm, go, ge = rows[state]
            f, nxt = Fm[v][j], None
            for p in sorted(preds[v], key=rank.get, reverse=high_rank):
                if H[p][j] + go == f:
                    nxt = (p, "H")
                    break
                if Fm[p][j] + ge == f:
                    nxt = (p, state)
                    break
            if nxt is None:
                break
            v, state = nxt
        else:
            Em, go, ge = rows[state]
            opened = H[v][j - 1] + go == Em[v][j]
            j -= 1
            if j == 0:
                break
            if opened:
                state = "H"
    return aln


def add_read_no_ring(graph, read, aln):
    """the no_ring mutant of rule 7: an aligned base that differs from its node makes a new node of no group"""
    prev = -1
    for j, c in enumerate(read):
        a = aln[j]
        w = a if a >= 0 and graph.base[a] == c else graph.add_node(c)
        graph.count[w] += 1
        if prev >= 0:
            graph.add_edge(prev, w)
        prev = w


def literal_poa(reads, **mutant):
    """reads -> (consensus bases, per-base counts) with literal_align; rules 2, 7 and 8 are cm's"""
    g = cm.Graph()
    add = add_read_no_ring if mutant.get("no_ring") else cm.add_read
    for r in reads:
        add(g, r, literal_align(g, r, **mutant))
    return cm.consensus(g)


def node_distance(graph, rank, u, w):
    """edges on the shortest path u -> w, None if there is none"""
    if u == w:
        return 0
    seen, front, d = {u}, [u], 0
    while front:
        d += 1
        nxt = []
        for x in front:
            for e in graph.outs[x]:
                y = graph.e_to[e]
                if y == w:
                    return d
                if y not in seen and rank[y] < rank[w]:
                    seen.add(y)
                    nxt.append(y)
        front = nxt
    return None


def path_score(graph, read, aln, one_gap_type=False):
    """the rule-1 score of an alignment (aligned node per read position, -1: none) against the graph it was made on: +5 / -4 per aligned
    pair, gap_score(L) per maximal run of unaligned read bases between aligned ones and per run of L nodes skipped between consecutive
    aligned nodes (along the fewest edges); None if consecutive aligned nodes are not connected.  Nothing aligned scores 0."""
    pairs = [(j, v) for j, v in enumerate(aln) if v >= 0]
    if not pairs:
        return 0
    rank = {v: i for i, v in enumerate(graph.topo())}
    score = 0
    for k, (j, v) in enumerate(pairs):
        score += MATCH if graph.base[v] == read[j] else MISMATCH
        if k:
            pj, pv = pairs[k - 1]
            d = node_distance(graph, rank, pv, v)
            if d is None or d == 0:
                return None
            if j - pj > 1:
                score += gap_score(j - pj - 1, one_gap_type)
            if d > 1:
                score += gap_score(d - 1, one_gap_type)
    return score


def gap_runs(graph, aln):
    """-> (runs of unaligned read bases between aligned ones as (read position, length), runs of skipped nodes as (read position of the
    aligned base behind the run, length), aligned bases in front of the first run, aligned bases behind the last)"""
    pairs = [(j, v) for j, v in enumerate(aln) if v >= 0]
    rank = {v: i for i, v in enumerate(graph.topo())}
    ins, dels, marks = [], [], []
    for (pj, pv), (j, v) in zip(pairs, pairs[1:]):
        if j - pj > 1:
            ins.append((pj + 1, j - pj - 1))
            marks.append(j)
        d = node_distance(graph, rank, pv, v)
        if d > 1:
            dels.append((j, d - 1))
            marks.append(j)
    if not marks:
        return ins, dels, len(pairs), 0
    return ins, dels, sum(j < marks[0] for j, _ in pairs), sum(j >= marks[-1] for j, _ in pairs)


# ---- the model, traced ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_trace(reads, dtype="int64"):
    """cm.poa(reads) with what each alignment did: -> ((consensus, counts), [dict(best, e1_min, e2_min, score, score_one_type, ins, dels,
    left, right, nodes) per read]); computed once per process and shared"""
    g, recs = cm.Graph(), []
    for r in reads:
        out = {}
        aln = cm.align(g, r, out=out, dtype=np.dtype(dtype))
        out["score"] = path_score(g, r, aln)
        out["score_one_type"] = path_score(g, r, aln, one_gap_type=True)
        out["ins"], out["dels"], out["left"], out["right"] = gap_runs(g, aln)
        out["nodes"] = len(g.base)
        recs.append(out)
        cm.add_read(g, r, aln)
    stats = dict(max_group=max((len(x) for x in g.group), default=0), max_indeg=max((len(x) for x in g.ins), default=0), nodes=len(g.base))
    return cm.consensus(g), recs, stats


def model(reads):
    """(consensus bases, per-base counts) of a molecule, from the shared trace"""
    reads = tuple(reads)
    big = max((len(r) for r in reads), default=0) > 3000
    return model_trace(reads, "int32" if big else "int64")[0]


# ---- the device call --------------------------------------------------------------------------------------------------------------------
def batch(mols):
    seqs = b"".join(r for m in mols for r in m)
    read_off = np.zeros(sum(len(m) for m in mols) + 1, dtype=np.uint64)
    read_off[1:] = np.cumsum([len(r) for m in mols for r in m])
    mol_off = np.zeros(len(mols) + 1, dtype=np.int32)
    mol_off[1:] = np.cumsum([len(m) for m in mols])
    return np.frombuffer(seqs, dtype=np.uint8).copy(), read_off, mol_off


def check_poa(lib, ctx, mols, max_ps=20, stats=False, **kw):
    """smi_poa_batch over mols: consensus and QV bytes equal the model's for every molecule -> molecules run again (with stats=True: that and
    the call's statistics)"""
    got = lib.poa_batch(ctx, *batch(mols), max_ps=max_ps, stats=stats, **kw)
    cons, qvs, rerun = got[0], got[1], got[3]
    for i, m in enumerate(mols):
        want, same = model(m)
        wq = bytes(cm.qv_byte(s, len(m), max_ps) for s in same)
        assert (cons[i], qvs[i]) == (want, wq), f"molecule {i}: {len(m)} reads of {[len(r) for r in m]} bases"
    return (rerun, got[4]) if stats else rerun


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def fit(rng, s, n):
    """s cut or padded with random bases to exactly n"""
    return s[:n] if len(s) >= n else s + cm.random_seq(rng, n - len(s))


SEAM_N = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)
RUN_L = (1, 2, 3, 4, 63, 64, 65, 130)
RUN_P = (62, 63, 64, 65, 127, 128, 129, 192)


def seam_lengths():
    out = {}
    for n in SEAM_N:
        rng = _rng(f"seam{n}")
        src = cm.random_seq(rng, n)
        out[f"seam-n{n}"] = (src,) + tuple(fit(rng, cm.noisy_copy(rng, src, 0.1), k) for k in (n, n - 1, n + 1))
    return out


def bridged(flank_left, flank_right, length):
    """both flanks of a gap stay in a local alignment when the shorter one earns more than the gap costs"""
    return 5 * min(flank_left, flank_right) > -gap_score(length)


def other_base(b):
    return b"C" if b == b"A" else b"A"


def ins_runs(n_src=400):
    """source, source with L random bases inserted at read position p, two clean copies; the inserted run starts and ends with a base that
    differs from the source's next one, so the gap has one place to be"""
    out = {}
    for L in RUN_L:
        for p in RUN_P:
            if p >= n_src or not bridged(p, n_src - p, L) or (L == 130 and p == 192):
                continue
            rng = _rng(f"ins{n_src}-{L}-{p}")
            src = cm.random_seq(rng, n_src)
            run = bytearray(cm.random_seq(rng, L))
            run[0] = other_base(src[p:p + 1])[0] if run[0] == src[p] else run[0]
            run[-1] = other_base(src[p - 1:p])[0] if run[-1] == src[p - 1] else run[-1]
            if L == 1 and (run[0] == src[p] or run[0] == src[p - 1]):
                run[0] = next(b for b in b"ACGT" if b not in (src[p], src[p - 1]))
            out[f"ins{n_src}-L{L}-p{p}"] = (src, src[:p] + bytes(run) + src[p:], src, src)
    return out


def del_runs(n_src=400):
    """source, source without src[p:p+L], two clean copies; per L one more where the second read puts a substitution inside the stretch
    before the deletion is aligned, so that F walks through a bubble"""
    out = {}
    bubble_p = 128 if n_src >= 400 else 64
    for L in RUN_L:
        for p in RUN_P:
            if p + L >= n_src or (L == 130 and p == 192):
                continue
            open_end = not bridged(p, n_src - p - L, L)        # the shorter flank earns less than the gap costs: only one flank aligns
            if open_end and n_src < 400:
                continue
            rng = _rng(f"del{n_src}-{L}-{p}")
            src = bytearray(cm.random_seq(rng, n_src))
            # one place for the gap: the bases on both sides of the stretch differ from the stretch's own ends
            if src[p - 1] == src[p + L - 1]:
                src[p - 1] = other_base(bytes(src[p + L - 1:p + L]))[0]
            if src[p + L] == src[p]:
                src[p + L] = other_base(bytes(src[p:p + 1]))[0]
            src = bytes(src)
            cut = src[:p] + src[p + L:]
            out[f"del{n_src}-L{L}-p{p}" + ("-unbridged" if open_end else "")] = (src, cut, src, src)
            if p == bubble_p:
                k = p + L // 2
                sub = src[:k] + other_base(src[k:k + 1]) + src[k + 1:]
                out[f"del{n_src}-L{L}-p{p}-bubble"] = (src, sub, cut, src)
    out.update(gap_ties())
    return out


def gap_ties():
    """short, very noisy molecules (35 % errors) in which an F1 and an F2 (or E1 and E2) of equal value come from gaps of different
    lengths, so that the order rule 6 tries them in decides which bases align: found by search, they are what notices F2 tried before F1"""
    out = {}
    for seed in (26, 41, 50):
        rng = np.random.default_rng(seed)
        src = cm.random_seq(rng, int(rng.integers(20, 50)))
        out[f"gap-ties-{seed}"] = tuple(cm.noisy_copy(rng, src, 0.35) for _ in range(5))
    return out


def low_complexity():
    return {"homopolymer-A": (b"A" * 130, b"A" * 70, b"A" * 200, b"A" * 64),
            "dinucleotide-AC": (b"AC" * 100, b"AC" * 64 + b"A", b"CA" * 90),
            "disjoint-ACG": (b"A" * 100, b"C" * 100, b"G" * 100)}


def wide_groups():
    rng = _rng("wide")
    src = cm.random_seq(rng, 80)
    out = {"wide-20": tuple(src[:40] + bytes([128 + k, 200 - k]) + src[42:] for k in range(20))}
    # two more reads that pair read 3's first byte with read 7's second: no edge joins those two nodes, so the second byte is aligned to a
    # node of another base and has to be found by walking that node's group
    crossed = src[:40] + bytes([128 + 3, 200 - 7]) + src[42:]
    out["wide-20-crossed"] = out["wide-20"] + (crossed, crossed)
    every = bytes(range(256))
    perm = bytes(rng.permutation(256).astype(np.uint8))
    out["all-bytes"] = (every, every[:100] + perm[:8] + every[108:], every[10:200], cm.noisy_copy(rng, every, 0.1, every), perm, every)
    # arms of unequal length between the same two nodes: a tie between predecessors decides which column the next read's base joins
    a, b = src[:30], src[50:]
    out["unequal-arms"] = (a + b"AC" + b, a + b"G" + b, a + b"T" + b, a + b"TT" + b, a + b"AC" + b)
    return out


def many_reads():
    rng = _rng("many")
    src = cm.random_seq(rng, 60)
    return {"many-70": tuple(fit(rng, cm.noisy_copy(rng, src, 0.1), 60) for _ in range(70))}


def int16_extreme():
    rng = _rng("int16")
    big = cm.random_seq(rng, 6000)
    return {"int16-6000": (big, big, big[2000:2100], cm.noisy_copy(rng, big[5800:]))}


FAMILIES = {"seam_lengths": seam_lengths, "ins_runs": ins_runs, "del_runs": del_runs, "low_complexity": low_complexity,
            "wide_groups": wide_groups, "many_reads": many_reads, "int16_extreme": int16_extreme}


@functools.lru_cache(maxsize=None)
def family(name, *args):
    """{case id: molecule (a tuple of reads)} of a family, built once per process"""
    return FAMILIES[name](*args)
