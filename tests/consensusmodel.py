"""Plain-Python / numpy model of `ComputeConsensus` (ComputeConsensus.java:L67-107 over LongreadParser, LongreadRecord.fromSAMRecord,
Longread, MoleculeDataset.callConsensus, Consensus.call and ConsensusMsa.process) with this build's POA: the
consensus FASTQ of an inflated BAM, byte for byte what the library writes.  Test infrastructure only."""
import importlib
import math
import struct

import numpy as np

import __graft_entry__ as graft

MATCH, MISMATCH, G, E, Q, C = 5, -4, -8, -6, -10, -4
NEG = -1_000_000_000

DEFAULTS = dict(cell_tag="BC", umi_tag="U8", gene_tag="IG", tso_end_tag="TE", polya_start_tag="PS", cdna_tag="CS", us_tag="US", rn_tag="RN",
                max_clip=150, mapqv0=False, max_reads=20, min_ps=3, max_ps=20)
COUNT_KEYS = ("records", "valid", "unvalid", "mapqv0", "no_gene", "no_umi", "chimeria", "null", "reads", "reads_multi", "molecules")


class ConsensusError(RuntimeError):
    pass


# ---- the POA ----------------------------------------------------------------------------------------------------------------------------
class Graph:
    def __init__(self):
        self.base, self.count, self.group = [], [], []     # group: the node's aligned group, a shared list
        self.ins, self.outs = [], []                       # lists of edge ids
        self.e_from, self.e_to, self.e_w = [], [], []

    def add_node(self, b, group_of=None):
        v = len(self.base)
        self.base.append(b)
        self.count.append(0)
        self.ins.append([])
        self.outs.append([])
        if group_of is None:
            self.group.append([v])
        else:
            g = self.group[group_of]
            g.append(v)
            self.group.append(g)
        return v

    def add_edge(self, u, w):
        for e in self.outs[u]:
            if self.e_to[e] == w:
                self.e_w[e] += 1
                return
        e = len(self.e_from)
        self.e_from.append(u)
        self.e_to.append(w)
        self.e_w.append(1)
        self.outs[u].append(e)
        self.ins[w].append(e)

    def topo(self):
        """Kahn's sort, always taking the ready node with the smallest creation id (rule 3)"""
        import heapq

        n = len(self.base)
        indeg = [len(x) for x in self.ins]
        ready = [v for v in range(n) if indeg[v] == 0]
        heapq.heapify(ready)
        order = []
        while ready:
            v = heapq.heappop(ready)
            order.append(v)
            for e in self.outs[v]:
                w = self.e_to[e]
                indeg[w] -= 1
                if indeg[w] == 0:
                    heapq.heappush(ready, w)
        if len(order) != n:
            raise ConsensusError("POA graph has a cycle")
        return order

    def preds(self, v):
        return [self.e_from[e] for e in self.ins[v]]


def align(graph, read, out=None, dtype=np.int64):
    """read (bytes) against the graph -> aligned node per read position (-1: not aligned), rules 1 and 3-6.  out: a dict that receives
    `best` (H of the end cell, 0 when nothing aligns), `e1_min` / `e2_min` (the smallest E1 / E2 of the alignment, None without a DP);
    dtype: the matrices' type (int32 holds every value: |H'[k] - k e| <= 5 n + 6 n)"""
    n, N = len(read), len(graph.base)
    aln = [-1] * n
    if out is not None:
        out.update(best=0, e1_min=None, e2_min=None)
    if n == 0 or N == 0:
        return aln
    order = graph.topo()
    rank = [0] * N
    for i, v in enumerate(order):
        rank[v] = i
    rd = np.frombuffer(read, dtype=np.uint8).astype(dtype)
    jj = np.arange(1, n + 1, dtype=dtype)
    H, F1, F2, E1, E2 = (np.zeros((N, n), dtype=dtype) for _ in range(5))
    preds = [graph.preds(v) for v in range(N)]
    best, bv, bj = 0, -1, -1
    for v in order:
        sc = np.where(rd == graph.base[v], MATCH, MISMATCH)
        ps = preds[v]
        if not ps:
            M = sc.copy()
            f1 = np.full(n, G, dtype=dtype)
            f2 = np.full(n, Q, dtype=dtype)
        else:
            hp = H[ps]
            hs = np.concatenate([np.zeros((len(ps), 1), dtype=dtype), hp[:, :-1]], axis=1)
            M = hs.max(axis=0) + sc
            f1 = np.maximum(hp + G, F1[ps] + E).max(axis=0)
            f2 = np.maximum(hp + Q, F2[ps] + C).max(axis=0)
        h1 = np.maximum(np.maximum(M, 0), np.maximum(f1, f2))          # H' = max(0, M, F1, F2)
        # E[j] = max over k < j of H'[k] + g + (j-1-k) e, H'[0] = 0: a prefix maximum of H'[k] - k e
        e1 = G + (jj - 1) * E + np.maximum.accumulate(np.concatenate([[0], h1[:-1] - jj[:-1] * E]))
        e2 = Q + (jj - 1) * C + np.maximum.accumulate(np.concatenate([[0], h1[:-1] - jj[:-1] * C]))
        h = np.maximum(h1, np.maximum(e1, e2))
        H[v], F1[v], F2[v], E1[v], E2[v] = h, f1, f2, e1, e2
        m = int(h.max())
        if m > best:
            best, bv, bj = m, v, int(np.argmax(h)) + 1
    if out is not None:
        out.update(best=best, e1_min=int(E1.min()), e2_min=int(E2.min()))
    if best <= 0:
        return aln

    def m_of(v, j):
        s = MATCH if graph.base[v] == read[j - 1] else MISMATCH
        ps = preds[v]
        if not ps:
            return s, -1
        vals = [(int(H[p][j - 2]) if j >= 2 else 0) + s for p in ps]
        mx = max(vals)
        p = min((rank[p], p) for p, x in zip(ps, vals) if x == mx)[1]
        return mx, p

    def hprime(v, j):
        if j == 0:
            return 0
        return max(0, m_of(v, j)[0], int(F1[v][j - 1]), int(F2[v][j - 1]))

    v, j, state = bv, bj, "H"
    while True:
        if state in ("H", "H'"):
            mval, p = m_of(v, j)
            f1, f2 = int(F1[v][j - 1]), int(F2[v][j - 1])
            h = int(H[v][j - 1]) if state == "H" else max(0, mval, f1, f2)
            if h == 0:
                break
            if h == mval:
                aln[j - 1] = v
                if p < 0 or j == 1:
                    break
                v, j, state = p, j - 1, "H"
            elif h == f1:
                state = "F1"
            elif h == f2:
                state = "F2"
            elif h == int(E1[v][j - 1]):
                state = "E1"
            else:
                state = "E2"
        elif state in ("F1", "F2"):
            go, ge, Fm = (G, E, F1) if state == "F1" else (Q, C, F2)
            f = int(Fm[v][j - 1])
            nxt = None
            for p in sorted(preds[v], key=lambda x: rank[x]):
                if int(H[p][j - 1]) + go == f:
                    nxt = (p, "H")
                    break
                if int(Fm[p][j - 1]) + ge == f:
                    nxt = (p, state)
                    break
            if nxt is None:
                break
            v, state = nxt
        else:
            go, ge, Em = (G, E, E1) if state == "E1" else (Q, C, E2)
            f = int(Em[v][j - 1])
            opened = hprime(v, j - 1) + go == f
            j -= 1
            if j == 0:
                break
            state = "H'" if opened else state
    return aln


def add_read(graph, read, aln):
    """rule 7: the read's path through the graph; counts and edge weights +1 -> the path (node ids)"""
    prev, path = -1, []
    for j, c in enumerate(read):
        a = aln[j]
        w = -1
        if a >= 0:
            for u in graph.group[a]:
                if graph.base[u] == c:
                    w = u
                    break
            if w < 0:
                w = graph.add_node(c, group_of=a)
        else:
            w = graph.add_node(c)
        graph.count[w] += 1
        if prev >= 0:
            graph.add_edge(prev, w)
        prev = w
        path.append(w)
    return path


def consensus(graph):
    """rule 8, heaviest bundle -> (bases, per-base read counts)"""
    N = len(graph.base)
    if N == 0:
        return b"", []
    order = graph.topo()
    rank = [0] * N
    for i, v in enumerate(order):
        rank[v] = i
    score, pred = [0] * N, [-1] * N
    for v in order:
        bk = None
        for e in graph.ins[v]:
            p = graph.e_from[e]
            k = (graph.e_w[e], score[p], -rank[p])
            if bk is None or k > bk:
                bk, pred[v] = k, p
        score[v] = 0 if bk is None else bk[0] + score[pred[v]]
    end, bs = -1, -1
    for v in order:
        if score[v] > bs:
            bs, end = score[v], v
    path = []
    v = end
    while v >= 0:
        path.append(v)
        v = pred[v]
    path.reverse()
    v = end
    while graph.outs[v]:
        v = graph.e_to[max(graph.outs[v], key=lambda e: (graph.e_w[e], -rank[graph.e_to[e]]))]
        path.append(v)
    return bytes(graph.base[v] for v in path), [graph.count[v] for v in path]


def poa(reads, dtype=np.int64):
    """reads (bytes, selection order) -> (consensus bases, per-base counts)"""
    g = Graph()
    for r in reads:
        add_read(g, r, align(g, r, dtype=dtype))
    return consensus(g)


def qv_byte(same, rows, max_ps):
    """ConsensusMsa.process L68-80: f = same / rows; MAXPS when all agree, else 33 + Math.round(-10 log10(1 - f)) (floor(x + 0.5))"""
    f = same / rows
    if f == 1.0:
        return 33 + max_ps
    return 33 + int(math.floor(-10 * math.log10(1.0 - f) + 0.5))


def molecule_consensus(reads, min_ps, max_ps):
    """Consensus.call L189-232 -> (cons bytes, qv bytes)"""
    if len(reads) == 1:
        return reads[0], bytes([33 + min_ps]) * len(reads[0])
    if len(reads) == 2:
        s1, s2 = reads
        cons = s1 if len(s1) > len(s2) else s2
        return cons, bytes([33 + min_ps]) * len(cons)
    cons, same = poa(reads)
    return cons, bytes(qv_byte(s, len(reads), max_ps) for s in same)


# ---- the records ------------------------------------------------------------------------------------------------------------------------
def _split_aux(aux):
    graft.load_package()
    au = importlib.import_module(graft.PKG_NAME + ".assignumis")
    out = {}
    for tag, raw in au.split_aux(aux):
        out[tag] = raw                                   # htsjdk keeps a repeated tag's last value
    return out


_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


def _value(raw, want, name, tag):
    """getAttribute + the reference's cast: a value of another type aborts the parse (ClassCastException)"""
    if raw is None:
        return None
    ty = chr(raw[2])
    if want == "Z" and ty == "Z":
        return raw[3:-1]
    if want == "i" and ty in _INT:
        v = struct.unpack(_INT[ty], raw[3:])[0]
        if v <= 0x7FFFFFFF:
            return v
    if want == "f" and ty == "f":
        return struct.unpack("<f", raw[3:])[0]
    raise ConsensusError(f"read {name}: attribute {tag} of type {ty} is not the type ComputeConsensus reads")


def float_key(x):
    """Float.compare order: -0.0 < 0.0, NaN above everything"""
    if x != x:
        return (1, 0.0, 0)
    return (0, x, 0 if (x == 0 and math.copysign(1, x) < 0) else 1)


def parse_records(bam, cfg):
    """LongreadParser over an inflated BAM -> (kept records in file order, counts)"""
    import bammodel

    _text, _refs, recs = bammodel.parse_bam(bam)
    cnt = dict.fromkeys(COUNT_KEYS, 0)
    kept = []
    for r in recs:
        cnt["records"] += 1
        name = r["name"]
        aux = _split_aux(r["aux"])
        get = lambda tag, want: _value(aux.get(tag), want, name, tag)  # noqa: E731
        get(cfg["gene_tag"], "Z")
        bc = get(cfg["cell_tag"], "Z")
        umi = get(cfg["umi_tag"], "Z")
        if bc is None or r["flag"] & 4:
            cnt["unvalid"] += 1
            cnt["null"] += 1
            continue
        bc = bc.replace(b"-1", b"")
        de = get("de", "f")
        if de is None:
            de = get("df", "f")
        if de is None:
            de = 1.0
        get(cfg["rn_tag"], "i")
        if not r["cigar"]:
            raise ConsensusError(f"read {name}: no CIGAR")
        first, last = r["cigar"][0], r["cigar"][-1]
        chim = (first[0] in "SH" and first[1] > cfg["max_clip"]) or (last[0] in "SH" and last[1] > cfg["max_clip"])
        if chim:
            cnt["unvalid"] += 1
            cnt["chimeria"] += 1
            continue
        cdna = get(cfg["cdna_tag"], "Z")
        if cdna is None:
            us = get(cfg["us_tag"], "Z")
            if us is None:
                raise ConsensusError(f"read {name}: neither {cfg['cdna_tag']} nor {cfg['us_tag']}")
            te = get(cfg["tso_end_tag"], "i") or 0
            ps = get(cfg["polya_start_tag"], "i") or 0
            end = ps if (ps != 0 and ps < len(us) - 1) else len(us) - 1
            if te < end and te < 0:
                raise ConsensusError(f"read {name}: {cfg['tso_end_tag']} {te} is outside {cfg['us_tag']}")   # String.substring throws
            cdna = us[te:end] if te < end else us
        if umi is None:
            cnt["unvalid"] += 1
            cnt["no_umi"] += 1
            continue
        if not cfg["mapqv0"] and r["mapq"] == 0 and r["flag"] & 0x900:
            cnt["unvalid"] += 1
            cnt["mapqv0"] += 1
            continue
        cnt["valid"] += 1
        kept.append(dict(name=name, bc=bc, umi=umi, de=de, cdna=cdna))
    return kept, cnt


def molecules(kept, max_reads, cnt):
    """Longread / MoleculeDataset / Consensus(name, longreads, true) -> [(name, [selected cDNAs])] in order of first kept record"""
    reads = {}
    for k in kept:
        reads.setdefault(k["name"], []).append(k)
    cnt["reads"] = len(reads)
    cnt["reads_multi"] = sum(len(v) > 1 for v in reads.values())
    mols = {}
    for name, recs in reads.items():                      # dict order = first kept record
        best = sorted(recs, key=lambda x: float_key(x["de"]))[0]
        last = recs[-1]
        mols.setdefault(last["bc"] + b":" + last["umi"], (last["bc"], last["umi"], []))[2].append(best)
    cnt["molecules"] = len(mols)
    out = []
    for bc, umi, rs in mols.values():
        sel = sorted(rs, key=lambda x: float_key(x["de"]))[:max_reads]
        out.append((bc + b"-" + umi + b"-" + str(len(rs)).encode(), [x["cdna"] for x in sel]))
    return out


def compute_consensus(bam, **kw):
    """-> (FASTQ bytes, counts)"""
    cfg = dict(DEFAULTS, **kw)
    kept, cnt = parse_records(bam, cfg)
    out = []
    for name, sel in molecules(kept, cfg["max_reads"], cnt):
        cons, qv = molecule_consensus(sel, cfg["min_ps"], cfg["max_ps"])
        out.append(b"@" + name + b"\n" + cons + b"\n+\n" + qv + b"\n")
    return b"".join(out), cnt


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------
def noisy_copy(rng, src, rate=0.07, alphabet=b"ACGT"):
    """ONT-like copy of src: substitutions, insertions and deletions, each about rate / 3"""
    out = bytearray()
    for b in src:
        x = rng.random()
        if x < rate / 3:
            out.append(alphabet[rng.integers(len(alphabet))])
        elif x < 2 * rate / 3:
            out.append(b)
            out.append(alphabet[rng.integers(len(alphabet))])
        elif x < rate:
            continue
        else:
            out.append(b)
    return bytes(out)


def random_seq(rng, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)])
