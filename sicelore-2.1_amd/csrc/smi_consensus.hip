// smi_consensus.hip -- `ComputeConsensus` (org/ipmc/sicelore/programs/ComputeConsensus.java:L67-107): K-POA on the device, the record
// parser, the molecule grouping and the FASTQ writer on the host.
//
// Host, in the reference's order:
//   records   LongreadParser.parseSAMRecord (LongreadParser.java:L96-115) over LongreadRecord.fromSAMRecord (LongreadRecord.java:L71-195):
//             null / unmapped -> "-1" removed from the barcode -> chimeric (first or last CIGAR operation S/H longer than MAXCLIP, L108-112)
//             -> cDNA (CDNATAG, else USTAG[TE:end] with end = PS if 0 < PS < len-1 else len-1, L116-135) -> no UMI -> mapq 0 and
//             secondary / supplementary unless MAPQV0 (L105-112).  A value of another type than the reference casts to, a mapped record
//             without CIGAR, or a kept record with neither cDNA tag aborts the reference's parse loop (L80-82): here it fails the call
//             with the read's name.
//   reads     Longread.addRecord / getBestRecord (Longread.java:L40-60): best record = lowest `de` in Float.compare order, stable;
//             barcode and UMI from the last kept record.
//   molecules MoleculeDataset(LongreadParser) L60-98 keyed `barcode:umi`; Consensus(name, longreads, true) L52-69: reads by their best
//             record's `de`, stable (the reference's ties are THashMap order; here the order of each read's first kept record), the first
//             min(MAXREADS, n); name BC-UMI-n (MoleculeDataset.callConsensus L666).  Molecules are written in the order of their first
//             kept record (the reference: hash order).
//   output    Consensus.call L189-232: 1 read -> its cDNA, 2 -> s1 if len(s1) > len(s2) else s2, both with MINPS; 3 or more -> K-POA
//             and ConsensusMsa.process L59-87's QVs from per-node read counts.
// K-POA: one wavefront per molecule, persistent waves taking molecules largest first from an atomic counter.  For every read in
// selection order: Kahn's sort (smallest creation id first) -> the local-alignment DP with convex gaps over the graph (read positions
// striped over the lanes, the E recurrences as a prefix maximum across the wave) -> traceback -> the read's path added to the graph;
// then the heaviest bundle and per-base read counts.  Graph, DP matrices and traceback scratch live in the wave's slot of a per-launch
// arena in HBM.  The rules are DESIGN.md section 8c's; tests/consensusmodel.py implements the same ones.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "smi_handle.h"
#include "smi_internal.h"

namespace smi {
namespace {

constexpr int kMatch = 5, kMismatch = -4, kG = -8, kE = -6, kQ = -10, kC = -4;  // spoa -r 2 defaults (ComputeConsensus exposes no options)
constexpr int kNeg = -1000000000;                                                 // -inf: k * e and additions stay inside int32
constexpr int kGraphInts = 16;  // int arrays of node_cap entries in a slot (nodes 11, edges 5)
constexpr int kStOverflow = 1, kStCycle = 2;
// DP rows are stored as int16 when every read of the launch has at most kNarrowMaxLen bases, else as int32.  The cells the recurrences and
// the traceback read are exact in int16.  The bound that matters is the upper one: a local alignment of n read bases scores at most 5 n, so
// H <= 5 n <= 30000.  Below, nothing goes under -10: H' >= 0, so F >= min(g, q), and E is g (q) plus a prefix maximum of
// H'[k] + (j - 1 - k) e over k = 0 .. j - 1 that contains k = j - 1, hence E1 >= g and E2 >= q.  The clamp at kStoreMin16 in store_e is therefore
// never reached; it is kept as it was (tests/test_poa_edges_cpu.py asserts both lower bounds on the model, test_poa_edges_gpu.py runs a
// 6,000 x 6,000 alignment whose H reaches exactly 30000)
constexpr int kNarrowMaxLen = 6000;
constexpr int kStoreMin16 = -30000;

template <class S>
__device__ __forceinline__ S store_e(int x) {
    return sizeof(S) == 2 ? (S)max(x, kStoreMin16) : (S)x;
}

struct Slot {
    int *base, *cnt, *grp, *in_head, *out_head, *indeg, *rank, *order, *heap, *score, *pred;
    int *e_from, *e_to, *e_w, *e_nin, *e_nout;
    int *aln;
    int *mat;
    size_t mat_cells;
};

struct PoaArgs {
    const uint8_t *seq;
    const uint64_t *read_off;   // n_reads + 1
    const int32_t *mol_off;     // n_mol + 1 (reads of molecule m: mol_off[m] .. mol_off[m + 1])
    const int32_t *mol_order;   // the order the waves take molecules in (largest first)
    int32_t n_mol;
    uint8_t *cons;              // molecule m's consensus at read_off[mol_off[m]] - read_off[0]
    uint32_t *same;             // its per-base read counts, same offsets
    int32_t *cons_len, *status;
    uint8_t *arena;
    size_t slot_bytes;
    int32_t node_cap, len_cap;
    unsigned *counter;
};

__device__ Slot slot_of(const PoaArgs &a, int w) {
    Slot s;
    int *p = (int *)(a.arena + (size_t)w * a.slot_bytes);
    const size_t nc = (size_t)a.node_cap;
    int **arr[] = {&s.base, &s.cnt, &s.grp, &s.in_head, &s.out_head, &s.indeg, &s.rank, &s.order, &s.heap, &s.score, &s.pred,
                   &s.e_from, &s.e_to, &s.e_w, &s.e_nin, &s.e_nout};
    for (int i = 0; i < kGraphInts; i++) *arr[i] = p + i * nc;
    s.aln = p + kGraphInts * nc;
    s.mat = s.aln + a.len_cap;
    const size_t used = (kGraphInts * nc + (size_t)a.len_cap) * sizeof(int);
    s.mat_cells = (a.slot_bytes - used) / sizeof(int);
    return s;
}

// Kahn's sort taking the ready node with the smallest id (a binary min-heap); every lane enters, lane 0 sorts.  -> nodes emitted
__device__ int topo_sort(Slot &s, int N, int lane) {
    __shared__ int emitted;
    for (int v = lane; v < N; v += 64) {
        int d = 0;
        for (int e = s.in_head[v]; e >= 0; e = s.e_nin[e]) d++;
        s.indeg[v] = d;
    }
    __syncthreads();
    if (lane == 0) {
        int hn = 0;
        for (int v = 0; v < N; v++)
            if (s.indeg[v] == 0) s.heap[hn++] = v;  // pushed in increasing order: already a heap
        int k = 0;
        while (hn > 0) {
            const int v = s.heap[0];
            const int last = s.heap[--hn];
            int i = 0;  // sift the last entry down from the root
            while (true) {
                int c = 2 * i + 1;
                if (c >= hn) break;
                if (c + 1 < hn && s.heap[c + 1] < s.heap[c]) c++;
                if (s.heap[c] >= last) break;
                s.heap[i] = s.heap[c];
                i = c;
            }
            if (hn > 0) s.heap[i] = last;
            s.order[k] = v;
            s.rank[v] = k++;
            for (int e = s.out_head[v]; e >= 0; e = s.e_nout[e]) {
                const int w = s.e_to[e];
                if (--s.indeg[w] == 0) {
                    int j = hn++;  // sift up
                    while (j > 0 && s.heap[(j - 1) / 2] > w) {
                        s.heap[j] = s.heap[(j - 1) / 2];
                        j = (j - 1) / 2;
                    }
                    s.heap[j] = w;
                }
            }
        }
        emitted = k;
    }
    __syncthreads();
    return emitted;
}

// M at (v, j) (rule 4) and the lowest-rank predecessor that gives it (-1: the virtual row of a node without predecessors)
template <class S>
__device__ void m_of(const Slot &s, const S *H, int n, int v, int j, uint8_t rb, int &M, int &p) {
    const int sc = s.base[v] == rb ? kMatch : kMismatch;
    M = kNeg;
    p = -1;
    if (s.in_head[v] < 0) {
        M = sc;
        return;
    }
    int pr = 0x7fffffff;
    for (int e = s.in_head[v]; e >= 0; e = s.e_nin[e]) {
        const int q = s.e_from[e];
        const int val = (j >= 2 ? H[(size_t)q * n + j - 2] : 0) + sc;
        if (val > M || (val == M && s.rank[q] < pr)) {
            M = val;
            p = q;
            pr = s.rank[q];
        }
    }
}

template <class S>
__device__ int hprime_at(const Slot &s, const S *H, const S *F1, const S *F2, int n, int v, int j, const uint8_t *rd) {
    if (j == 0) return 0;
    int M, p;
    m_of(s, H, n, v, j, rd[j - 1], M, p);
    const size_t c = (size_t)v * n + j - 1;
    return max(max(M, 0), max((int)F1[c], (int)F2[c]));
}

// one read against the graph: DP (all lanes), best cell, traceback (lane 0) -> s.aln[0 .. n)
template <class S>
__device__ int align_read(Slot &s, int N, const uint8_t *rd, int n, int lane) {
    for (int j = lane; j < n; j += 64) s.aln[j] = -1;
    if (n == 0 || N == 0) {
        __syncthreads();
        return 0;
    }
    if (topo_sort(s, N, lane) != N) return kStCycle;
    const size_t cells = (size_t)N * n;
    if (5 * cells * sizeof(S) > s.mat_cells * sizeof(int)) return kStOverflow;
    S *H = (S *)s.mat, *F1 = H + cells, *F2 = F1 + cells, *E1 = F2 + cells, *E2 = E1 + cells;
    int bH = 0, bR = 0x7fffffff, bJ = 0;
    for (int idx = 0; idx < N; idx++) {
        const int v = s.order[idx];
        const uint8_t b = (uint8_t)s.base[v];
        const int ih = s.in_head[v];
        int carry1 = 0, carry2 = 0;  // max of H'[k] - k e over the columns left of this chunk (column 0: H' = 0)
        S *Hv = H + (size_t)v * n;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane + 1;
            const bool act = j <= n;
            const int sc = (act && rd[j - 1] == b) ? kMatch : kMismatch;
            int M, f1, f2;
            if (ih < 0) {
                M = sc;
                f1 = kG;
                f2 = kQ;
            } else {
                M = f1 = f2 = kNeg;
                if (act) {
                    for (int e = ih; e >= 0; e = s.e_nin[e]) {
                        const size_t row = (size_t)s.e_from[e] * n;
                        const int hj = H[row + j - 1];
                        const int hm = j >= 2 ? (int)H[row + j - 2] : 0;
                        M = max(M, hm + sc);
                        f1 = max(f1, max(hj + kG, F1[row + j - 1] + kE));
                        f2 = max(f2, max(hj + kQ, F2[row + j - 1] + kC));
                    }
                }
            }
            const int hp = max(max(M, 0), max(f1, f2));
            int x1 = act ? hp - j * kE : kNeg, x2 = act ? hp - j * kC : kNeg;  // inclusive prefix maximum across the wave
            for (int off = 1; off < 64; off <<= 1) {
                const int y1 = __shfl_up(x1, off, 64), y2 = __shfl_up(x2, off, 64);
                if (lane >= off) {
                    x1 = max(x1, y1);
                    x2 = max(x2, y2);
                }
            }
            const int p1 = __shfl_up(x1, 1, 64), p2 = __shfl_up(x2, 1, 64);
            const int ex1 = lane == 0 ? carry1 : max(carry1, p1), ex2 = lane == 0 ? carry2 : max(carry2, p2);
            const int e1 = kG + (j - 1) * kE + ex1, e2 = kQ + (j - 1) * kC + ex2;
            const int h = max(hp, max(e1, e2));
            if (act) {
                const size_t c = (size_t)v * n + j - 1;
                Hv[j - 1] = (S)h;
                F1[c] = (S)f1;
                F2[c] = (S)f2;
                E1[c] = store_e<S>(e1);
                E2[c] = store_e<S>(e2);
                if (h > bH) {
                    bH = h;
                    bR = idx;
                    bJ = j;
                }
            }
            carry1 = max(carry1, __shfl(x1, 63, 64));
            carry2 = max(carry2, __shfl(x2, 63, 64));
        }
        __syncthreads();  // this row is read by the rows of its successors
    }
    for (int off = 32; off > 0; off >>= 1) {  // the first strict maximum in (node order, j) (rule 5)
        const int oh = __shfl_xor(bH, off, 64), orr = __shfl_xor(bR, off, 64), oj = __shfl_xor(bJ, off, 64);
        if (oh > bH || (oh == bH && (orr < bR || (orr == bR && oj < bJ)))) {
            bH = oh;
            bR = orr;
            bJ = oj;
        }
    }
    if (lane == 0 && bH > 0) {  // traceback (rule 6)
        enum { SH, SHP, SF1, SF2, SE1, SE2 };
        int v = s.order[bR], j = bJ, st = SH;
        while (true) {
            const size_t c = (size_t)v * n + j - 1;
            if (st == SH || st == SHP) {
                int M, p;
                m_of(s, H, n, v, j, rd[j - 1], M, p);
                const int f1 = F1[c], f2 = F2[c];
                const int h = st == SH ? (int)H[c] : max(max(M, 0), max(f1, f2));
                if (h == 0) break;
                if (h == M) {
                    s.aln[j - 1] = v;
                    if (p < 0 || j == 1) break;
                    v = p;
                    j--;
                    st = SH;
                } else if (h == f1) {
                    st = SF1;
                } else if (h == f2) {
                    st = SF2;
                } else {
                    st = h == E1[c] ? SE1 : SE2;
                }
            } else if (st == SF1 || st == SF2) {
                const S *Fm = st == SF1 ? F1 : F2;
                const int go = st == SF1 ? kG : kQ, ge = st == SF1 ? kE : kC;
                const int f = Fm[c];
                int np = -1, nst = SH, pr = 0x7fffffff;
                for (int e = s.in_head[v]; e >= 0; e = s.e_nin[e]) {  // lowest rank first; opening before extending
                    const int q = s.e_from[e];
                    const size_t qc = (size_t)q * n + j - 1;
                    if (s.rank[q] >= pr) continue;
                    if (H[qc] + go == f) {
                        np = q;
                        nst = SH;
                        pr = s.rank[q];
                    } else if (Fm[qc] + ge == f) {
                        np = q;
                        nst = st;
                        pr = s.rank[q];
                    }
                }
                if (np < 0) break;
                v = np;
                st = nst;
            } else {
                const S *Em = st == SE1 ? E1 : E2;
                const int go = st == SE1 ? kG : kQ;
                const bool opened = hprime_at(s, H, F1, F2, n, v, j - 1, rd) + go == Em[c];
                j--;
                if (j == 0) break;
                if (opened) st = SHP;
            }
        }
    }
    __syncthreads();
    return 0;
}

__device__ int add_edge(Slot &s, int u, int w, int &NE) {
    for (int e = s.out_head[u]; e >= 0; e = s.e_nout[e])
        if (s.e_to[e] == w) {
            s.e_w[e]++;
            return 0;
        }
    const int e = NE++;
    s.e_from[e] = u;
    s.e_to[e] = w;
    s.e_w[e] = 1;
    s.e_nout[e] = s.out_head[u];
    s.out_head[u] = e;
    s.e_nin[e] = s.in_head[w];
    s.in_head[w] = e;
    return 0;
}

__device__ int new_node(Slot &s, int &N, int b, int group_of) {
    const int v = N++;
    s.base[v] = b;
    s.cnt[v] = 0;
    s.in_head[v] = s.out_head[v] = -1;
    if (group_of < 0) {
        s.grp[v] = v;
    } else {
        s.grp[v] = s.grp[group_of];
        s.grp[group_of] = v;
    }
    return v;
}

// rule 7, lane 0
__device__ void add_read(Slot &s, int &N, int &NE, const uint8_t *rd, int n) {
    int prev = -1;
    for (int j = 0; j < n; j++) {
        const int c = rd[j], a = s.aln[j];
        int w = -1;
        if (a >= 0) {
            int u = a;
            do {
                if (s.base[u] == c) {
                    w = u;
                    break;
                }
                u = s.grp[u];
            } while (u != a);
            if (w < 0) w = new_node(s, N, c, a);
        } else {
            w = new_node(s, N, c, -1);
        }
        s.cnt[w]++;
        if (prev >= 0) add_edge(s, prev, w, NE);
        prev = w;
    }
}

template <class S>
__global__ void __launch_bounds__(64) k_poa(PoaArgs a) {
    const int lane = threadIdx.x;
    Slot s = slot_of(a, blockIdx.x);
    __shared__ int mol, N, NE, status;
    while (true) {
        if (lane == 0) {
            const unsigned k = atomicAdd(a.counter, 1u);
            mol = k < (unsigned)a.n_mol ? a.mol_order[k] : -1;
            N = NE = status = 0;
        }
        __syncthreads();
        const int m = mol;
        if (m < 0) return;
        const uint64_t base_off = a.read_off[a.mol_off[m]] - a.read_off[0];
        for (int r = a.mol_off[m]; r < a.mol_off[m + 1]; r++) {
            const uint8_t *rd = a.seq + (a.read_off[r] - a.read_off[0]);
            const int n = (int)(a.read_off[r + 1] - a.read_off[r]);
            const int st = align_read<S>(s, N, rd, n, lane);
            if (st) {
                if (lane == 0) status = st;
                break;
            }
            if (lane == 0) add_read(s, N, NE, rd, n);
            __syncthreads();
        }
        __syncthreads();
        if (status == 0 && N > 0 && topo_sort(s, N, lane) != N) status = kStCycle;
        if (lane == 0) {
            int len = 0;
            if (status == 0 && N > 0) {  // heaviest bundle (rule 8)
                int end = -1, bs = -1;
                for (int k = 0; k < N; k++) {
                    const int v = s.order[k];
                    int bp = -1, bw = -1, bsc = 0;
                    for (int e = s.in_head[v]; e >= 0; e = s.e_nin[e]) {
                        const int p = s.e_from[e], w = s.e_w[e], sp = s.score[p];
                        if (bp < 0 || w > bw || (w == bw && (sp > bsc || (sp == bsc && s.rank[p] < s.rank[bp])))) {
                            bp = p;
                            bw = w;
                            bsc = sp;
                        }
                    }
                    s.pred[v] = bp;
                    s.score[v] = bp < 0 ? 0 : bw + bsc;
                    if (s.score[v] > bs) {
                        bs = s.score[v];
                        end = v;
                    }
                }
                for (int v = end; v >= 0; v = s.pred[v]) len++;
                uint8_t *co = a.cons + base_off;
                uint32_t *so = a.same + base_off;
                int i = len;
                for (int v = end; v >= 0; v = s.pred[v]) {
                    co[--i] = (uint8_t)s.base[v];
                    so[i] = (uint32_t)s.cnt[v];
                }
                for (int v = end; s.out_head[v] >= 0;) {  // on to a sink along the heaviest out-edges, ties to the lower rank
                    int bt = -1, bw = -1;
                    for (int e = s.out_head[v]; e >= 0; e = s.e_nout[e]) {
                        const int t = s.e_to[e], w = s.e_w[e];
                        if (bt < 0 || w > bw || (w == bw && s.rank[t] < s.rank[bt])) {
                            bt = t;
                            bw = w;
                        }
                    }
                    v = bt;
                    co[len] = (uint8_t)s.base[v];
                    so[len++] = (uint32_t)s.cnt[v];
                }
            }
            a.cons_len[m] = len;
            a.status[m] = status;
        }
        __syncthreads();
    }
}

int device_cus(int dev) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    return n;
}

// DP matrix cells of a molecule's slot.  exact: the worst case (the graph holds at most the bases of the reads before read k when read k is
// aligned); otherwise the first-pass estimate (a graph of at most 3 x the longest read), never above the worst case
size_t mat_cells(const uint64_t *read_off, int r0, int r1, bool exact) {
    size_t before = 0, mat = 0, len = 0;
    for (int r = r0; r < r1; r++) {
        const size_t n = read_off[r + 1] - read_off[r];
        mat = std::max(mat, before * n);
        before += n;
        len = std::max(len, n);
    }
    return 5 * (exact ? mat : std::min(mat, std::min(before, 3 * len) * len));
}

}  // namespace

// K-POA over a batch: host arrays in, consensus bases and per-base counts out (offsets of the molecules' reads).  Pass 1 gives each molecule a
// slot of its estimate; a molecule whose graph outgrows it, or whose estimate does not fit the budget, is run again in pass 2 in a slot of its
// worst case.  A molecule whose worst case does not fit the budget fails the call: *bad = its index in the batch and *why says why (on any
// other error *bad = -1 and the error text is set).  *n_rerun = molecules run in pass 2.  stats (may be null): SMI_POA_STATS entries,
// host arithmetic over the launches made.
int poa_batch(smi_ctx *ctx, const uint8_t *seq, const uint64_t *read_off, const int32_t *mol_off, int32_t n_mol, size_t budget, uint8_t *cons,
              uint32_t *same, int32_t *cons_len, float *kernel_ms, int32_t *n_rerun, int32_t *bad, std::string *why, int64_t *stats) {
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_rerun) *n_rerun = 0;
    if (stats) std::fill(stats, stats + SMI_POA_STATS, (int64_t)0);
    *bad = -1;
    if (n_mol <= 0) return SMI_OK;
    SMI_HIP(hipSetDevice(ctx->device));
    const int n_reads = mol_off[n_mol] - mol_off[0];
    const uint64_t total = read_off[mol_off[n_mol]] - read_off[mol_off[0]];
    if (budget == 0) {
        size_t fr = 0, tot = 0;
        SMI_HIP(hipMemGetInfo(&fr, &tot));
        budget = std::min<size_t>(fr / 2, (size_t)32 << 30);
    }
    hipStream_t st = ctx->stream;
    // device copies of the inputs (offsets rebased to the first read)
    const int r0 = mol_off[0];
    std::vector<uint64_t> roff(n_reads + 1);
    for (int r = 0; r <= n_reads; r++) roff[r] = read_off[r0 + r] - read_off[r0];
    std::vector<int32_t> moff(n_mol + 1);
    for (int m = 0; m <= n_mol; m++) moff[m] = mol_off[m] - r0;
    const uint8_t *seq0 = seq + read_off[r0];
    constexpr const char *kWho = "smi_poa_batch";  // (the two texts below replace the buffer's own)
    DevBuf<uint8_t> d_seq{kWho}, d_cons{kWho}, d_arena{kWho};
    DevBuf<uint64_t> d_roff{kWho};
    DevBuf<int32_t> d_moff{kWho}, d_order{kWho}, d_len{kWho}, d_status{kWho};
    DevBuf<uint32_t> d_same{kWho}, d_counter{kWho};
    int rc;
    if ((rc = d_seq.alloc(total)) || (rc = d_cons.alloc(total)) || (rc = d_same.alloc(total)) || (rc = d_roff.alloc(n_reads + 1)) ||
        (rc = d_moff.alloc(n_mol + 1)) || (rc = d_order.alloc(n_mol)) || (rc = d_len.alloc(n_mol)) || (rc = d_status.alloc(n_mol)) ||
        (rc = d_counter.alloc(1))) {
        set_error("smi_poa_batch: device allocation of the batch failed");
        return rc;
    }
    SMI_HIP(hipMemcpyAsync(d_seq.p, seq0, total, hipMemcpyHostToDevice, st));
    SMI_HIP(hipMemcpyAsync(d_roff.p, roff.data(), roff.size() * 8, hipMemcpyHostToDevice, st));
    SMI_HIP(hipMemcpyAsync(d_moff.p, moff.data(), moff.size() * 4, hipMemcpyHostToDevice, st));
    // per molecule: total bases (node cap), longest read, row width (int16 up to kNarrowMaxLen bases per read), pass-1 and worst-case cells
    std::vector<size_t> tot_m(n_mol), len_m(n_mol), cell_b(n_mol), est(n_mol), worst(n_mol);
    for (int m = 0; m < n_mol; m++) {
        size_t t = 0, l = 0;
        for (int r = moff[m]; r < moff[m + 1]; r++) {
            t += roff[r + 1] - roff[r];
            l = std::max<size_t>(l, roff[r + 1] - roff[r]);
        }
        tot_m[m] = t;
        len_m[m] = l;
        cell_b[m] = l <= (size_t)kNarrowMaxLen ? 2 : 4;
        est[m] = mat_cells(roff.data(), moff[m], moff[m + 1], false) * cell_b[m];
        worst[m] = mat_cells(roff.data(), moff[m], moff[m + 1], true) * cell_b[m];
    }
    std::vector<int32_t> order(n_mol);
    for (int m = 0; m < n_mol; m++) order[m] = m;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return est[x] > est[y]; });
    std::vector<int32_t> status(n_mol, 0), lens(n_mol, 0);
    const int max_waves = 8 * device_cus(ctx->device);
    Events ev;
    SMI_HIP(hipEventCreate(&ev.a));
    SMI_HIP(hipEventCreate(&ev.b));
    float ms_total = 0.f;
    // launches: groups of molecules of one row width, largest first
    std::vector<int32_t> todo = order;
    for (int pass = 0; pass < 2 && !todo.empty(); pass++) {
        std::vector<int32_t> again;
        auto need = [&](int m) { return pass == 0 ? est[m] : worst[m]; };
        auto slot_of_group = [&](size_t g0, size_t g1, size_t &node_cap, size_t &len_cap) {
            size_t mat = 0;
            node_cap = 0;
            len_cap = 0;
            for (size_t i = g0; i < g1; i++) {
                const int m = todo[i];
                node_cap = std::max(node_cap, tot_m[m] + 1);
                len_cap = std::max(len_cap, len_m[m]);
                mat = std::max(mat, need(m));
            }
            return ((kGraphInts * node_cap + len_cap) * sizeof(int) + mat + 255) & ~(size_t)255;
        };
        if (pass == 1) std::stable_sort(todo.begin(), todo.end(), [&](int x, int y) { return worst[x] > worst[y]; });
        size_t g0 = 0;
        while (g0 < todo.size()) {
            // the group: molecules of the first one's row width down to a quarter of its matrix size share its slot size
            const size_t need0 = need(todo[g0]);
            size_t g1 = g0 + 1;
            while (g1 < todo.size() && cell_b[todo[g1]] == cell_b[todo[g0]] && need(todo[g1]) * 4 >= need0) g1++;
            size_t node_cap, len_cap;
            size_t slot = slot_of_group(g0, g1, node_cap, len_cap);
            if (slot > budget && g1 > g0 + 1) {  // a larger node cap of a later molecule: the first one alone
                g1 = g0 + 1;
                slot = slot_of_group(g0, g1, node_cap, len_cap);
            }
            if (slot > budget) {
                const int m = todo[g0];
                if (pass == 0) {  // its estimate does not fit: its worst case decides in pass 2
                    again.push_back(m);
                    g0++;
                    continue;
                }
                *bad = m;
                *why = std::to_string(moff[m + 1] - moff[m]) + " reads, " + std::to_string(tot_m[m]) + " bases: needs " + std::to_string(slot >> 20) +
                       " MiB of POA scratch, more than the budget of " + std::to_string(budget >> 20) + " MiB";
                set_error(*why);
                return SMI_ERR_INVALID;
            }
            const int waves = (int)std::max<size_t>(1, std::min<size_t>({budget / slot, (size_t)max_waves, g1 - g0}));
            if ((rc = d_arena.alloc((size_t)waves * slot))) {
                set_error("smi_poa_batch: device allocation of " + std::to_string(((size_t)waves * slot) >> 20) + " MiB of POA scratch failed");
                return rc;
            }
            if (stats) {
                stats[SMI_POA_STAT_LAUNCHES]++;
                stats[SMI_POA_STAT_WAVES] += waves;
                stats[SMI_POA_STAT_SLOT_REUSE] += std::max<int64_t>(0, (int64_t)(g1 - g0) - waves);
                stats[SMI_POA_STAT_MAX_SLOT_BYTES] = std::max<int64_t>(stats[SMI_POA_STAT_MAX_SLOT_BYTES], (int64_t)slot);
            }
            SMI_HIP(hipMemcpyAsync(d_order.p, todo.data() + g0, (g1 - g0) * 4, hipMemcpyHostToDevice, st));
            SMI_HIP(hipMemsetAsync(d_counter.p, 0, 4, st));
            PoaArgs a;
            a.seq = d_seq.p;
            a.read_off = d_roff.p;
            a.mol_off = d_moff.p;
            a.mol_order = d_order.p;
            a.n_mol = (int32_t)(g1 - g0);
            a.cons = d_cons.p;
            a.same = d_same.p;
            a.cons_len = d_len.p;
            a.status = d_status.p;
            a.arena = d_arena.p;
            a.slot_bytes = slot;
            a.node_cap = (int32_t)node_cap;
            a.len_cap = (int32_t)len_cap;
            a.counter = d_counter.p;
            SMI_HIP(hipEventRecord(ev.a, st));
            if (cell_b[todo[g0]] == 2)
                hipLaunchKernelGGL(k_poa<int16_t>, dim3(waves), dim3(64), 0, st, a);
            else
                hipLaunchKernelGGL(k_poa<int32_t>, dim3(waves), dim3(64), 0, st, a);
            SMI_HIP(hipGetLastError());
            SMI_HIP(hipEventRecord(ev.b, st));
            SMI_HIP(hipMemcpyAsync(status.data(), d_status.p, n_mol * 4, hipMemcpyDeviceToHost, st));
            SMI_HIP(hipStreamSynchronize(st));
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) ms_total += ms;
            (void)hipFree(d_arena.p);
            d_arena.p = nullptr;
            for (size_t i = g0; i < g1; i++) {
                const int m = todo[i];
                if (status[m] == kStCycle || (status[m] == kStOverflow && pass == 1)) {
                    *bad = m;
                    *why = status[m] == kStCycle ? "the POA graph has a cycle" : "overflowed its worst-case slot";
                    set_error(*why);
                    return SMI_ERR_INVALID;
                }
                if (status[m] == kStOverflow) again.push_back(m);
            }
            g0 = g1;
        }
        if (pass == 0 && n_rerun) *n_rerun = (int32_t)again.size();
        todo.swap(again);
    }
    SMI_HIP(hipMemcpyAsync(lens.data(), d_len.p, n_mol * 4, hipMemcpyDeviceToHost, st));
    SMI_HIP(hipMemcpyAsync(cons, d_cons.p, total, hipMemcpyDeviceToHost, st));
    SMI_HIP(hipMemcpyAsync(same, d_same.p, total * 4, hipMemcpyDeviceToHost, st));
    SMI_HIP(hipStreamSynchronize(st));
    std::memcpy(cons_len, lens.data(), n_mol * 4);
    if (kernel_ms) *kernel_ms = ms_total;
    return SMI_OK;
}

// ConsensusMsa.process L68-80: f = same / rows; MAXPS when all agree, else 33 + Math.round(-10 log10(1 - f)) = floor(x + 0.5)
uint8_t qv_byte(uint32_t same, uint32_t rows, int max_ps) {
    const double f = (double)same / (double)rows;
    if (f == 1.0) return (uint8_t)(33 + max_ps);
    return (uint8_t)(33 + (int64_t)std::floor(-10.0 * std::log10(1.0 - f) + 0.5));
}

}  // namespace smi

using namespace smi;

extern "C" int smi_poa_batch_ex(smi_ctx *ctx, const uint8_t *seqs, const uint64_t *read_off, const int32_t *mol_off, int32_t n_mol, int32_t max_ps,
                                size_t scratch_bytes, uint8_t *cons, uint8_t *qv, int32_t *cons_len, float *kernel_ms, int32_t *n_rerun,
                                int64_t *stats) {
    if (stats) std::fill(stats, stats + SMI_POA_STATS, (int64_t)0);
    if (!ctx || !read_off || !mol_off || n_mol < 0 || (n_mol && (!cons || !qv || !cons_len))) {
        set_error("smi_poa_batch: null argument");
        return SMI_ERR_INVALID;
    }
    if (n_mol == 0) return SMI_OK;
    if (mol_off[0] != 0 || read_off[0] != 0) {
        set_error("smi_poa_batch: mol_off[0] and read_off[0] must be 0");
        return SMI_ERR_INVALID;
    }
    for (int m = 0; m < n_mol; m++)
        if (mol_off[m + 1] < mol_off[m]) {
            set_error("smi_poa_batch: mol_off must not decrease");
            return SMI_ERR_INVALID;
        }
    const int n_reads = mol_off[n_mol];
    for (int r = 0; r < n_reads; r++)
        if (read_off[r + 1] < read_off[r] || read_off[r + 1] - read_off[r] > 0x7fffffffull) {
            set_error("smi_poa_batch: read_off must not decrease, reads at most 2^31 - 1 bases");
            return SMI_ERR_INVALID;
        }
    if (n_reads > 0 && !seqs) {
        set_error("smi_poa_batch: null argument");
        return SMI_ERR_INVALID;
    }
    const uint64_t total = read_off[n_reads];
    std::vector<uint32_t> same(std::max<uint64_t>(total, 1));
    int32_t bad = -1;
    std::string why;
    const int rc = poa_batch(ctx, seqs, read_off, mol_off, n_mol, scratch_bytes, cons, same.data(), cons_len, kernel_ms, n_rerun, &bad, &why,
                             stats);
    if (rc) {
        if (bad >= 0) set_error("smi_poa_batch: molecule " + std::to_string(bad) + " (" + why + ")");
        return rc;
    }
    for (int m = 0; m < n_mol; m++) {
        const uint64_t o = read_off[mol_off[m]];
        const uint32_t rows = (uint32_t)(mol_off[m + 1] - mol_off[m]);
        for (int i = 0; i < cons_len[m]; i++) qv[o + i] = qv_byte(same[o + i], rows, max_ps);
    }
    return SMI_OK;
}

extern "C" int smi_poa_batch(smi_ctx *ctx, const uint8_t *seqs, const uint64_t *read_off, const int32_t *mol_off, int32_t n_mol, int32_t max_ps,
                             size_t scratch_bytes, uint8_t *cons, uint8_t *qv, int32_t *cons_len, float *kernel_ms, int32_t *n_rerun) {
    return smi_poa_batch_ex(ctx, seqs, read_off, mol_off, n_mol, max_ps, scratch_bytes, cons, qv, cons_len, kernel_ms, n_rerun, nullptr);
}

// ---- the records (lr::read_consensus in smi_longread.h), molecules and the FASTQ (host) -------------------------------------------------
using smi::lr::float_less;

struct smi_consensus {
    smi_ctx *ctx = nullptr;
    smi_consensus_config cfg = {};
    lr::TagSet tags;
    // kept records in file order: their strings back to back in `text`
    std::string text;
    std::vector<uint64_t> name_off, bc_off, umi_off, cdna_off;  // each string: [off, off + len) with len in the *_len arrays
    std::vector<uint32_t> name_len, bc_len, umi_len, cdna_len;
    std::vector<float> de;
    int64_t counts[SMI_CONSENSUS_COUNTS] = {};
    std::string fastq;
    bool ran = false;
};

extern "C" int smi_consensus_default_config(smi_consensus_config *cfg) {
    if (!cfg) {
        set_error("smi_consensus_default_config: null argument");
        return SMI_ERR_INVALID;
    }
    *cfg = {};
    const char *names[] = {"BC", "U8", "IG", "TE", "PS", "CS", "US", "RN"};
    char *dst[] = {cfg->cell_tag, cfg->umi_tag, cfg->gene_tag, cfg->tso_end_tag, cfg->polya_start_tag, cfg->cdna_tag, cfg->us_tag, cfg->rn_tag};
    for (int i = 0; i < 8; i++) std::memcpy(dst[i], names[i], 3);
    cfg->max_clip = 150;
    cfg->mapqv0 = 0;
    cfg->max_reads = 20;
    cfg->min_ps = 3;
    cfg->max_ps = 20;
    cfg->n_threads = 20;
    cfg->scratch_bytes = 0;
    return SMI_OK;
}

extern "C" int smi_consensus_create(smi_ctx *ctx, const smi_consensus_config *cfg, smi_consensus **out) {
    if (!ctx || !cfg || !out) {
        set_error("smi_consensus_create: null argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    const char *tags[] = {cfg->cell_tag, cfg->umi_tag, cfg->gene_tag, cfg->tso_end_tag, cfg->polya_start_tag, cfg->cdna_tag, cfg->us_tag, cfg->rn_tag};
    const char *what[] = {"CELLTAG", "UMITAG", "GENETAG", "TSOENDTAG", "POLYASTARTTAG", "CDNATAG", "USTAG", "RNTAG"};
    for (int i = 0; i < 8; i++)
        if (!valid_tag(tags[i])) {
            set_error(std::string(what[i]) + " must be two characters");
            return SMI_ERR_INVALID;
        }
    if (cfg->max_reads < 1) {
        set_error("MAXREADS must be at least 1");
        return SMI_ERR_INVALID;
    }
    if (cfg->min_ps < 0 || cfg->min_ps > 93 || cfg->max_ps < 0 || cfg->max_ps > 93) {
        set_error("MINPS and MAXPS must be 0 .. 93 (a FASTQ quality character)");
        return SMI_ERR_INVALID;
    }
    smi_consensus *h = new smi_consensus();
    h->ctx = ctx;
    h->cfg = *cfg;
    h->cfg.n_threads = std::max(1, std::min(cfg->n_threads, 256));
    h->tags.set(lr::kCell, cfg->cell_tag).set(lr::kUmi, cfg->umi_tag).set(lr::kGene, cfg->gene_tag).set(lr::kRn, cfg->rn_tag);
    h->tags.set(lr::kTe, cfg->tso_end_tag).set(lr::kPs, cfg->polya_start_tag).set(lr::kCs, cfg->cdna_tag).set(lr::kUs, cfg->us_tag);
    *out = h;
    return SMI_OK;
}

extern "C" int smi_consensus_free(smi_consensus *h) {
    delete h;
    return SMI_OK;
}

extern "C" int smi_consensus_add_segment(smi_consensus *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n) {
    if (!h || n < 0 || (n && (!bam || !recs))) {
        set_error("smi_consensus_add_segment: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->ran) {
        set_error("smi_consensus_add_segment: the molecules were already built (smi_consensus_run)");
        return SMI_ERR_STATE;
    }
    const lr::Segment seg = lr::read_segment("smi_consensus_add_segment", bam, n_bam, recs, n, h->cfg.n_threads,
                                             [&](const uint8_t *b, const smi_bam_record &r, lr::Record &out, std::string &err) {
                                                 lr::read_consensus(b, r, h->tags, h->cfg.max_clip, h->cfg.mapqv0, out, err);
                                             });
    if (!seg.refused.empty()) {
        set_error(seg.refused);
        return SMI_ERR_INVALID;
    }
    if (seg.first_error >= 0) {
        set_error("ComputeConsensus: read " + std::string(lr::read_name(bam, recs[seg.first_error])) + ": " + seg.error);
        return SMI_ERR_INVALID;
    }
    int64_t *c = h->counts;
    for (int32_t i = 0; i < n; i++) {
        const lr::Record &p = seg.recs[i];
        c[SMI_CC_RECORDS]++;
        if (p.what != lr::kKept) {
            c[SMI_CC_UNVALID]++;
            c[p.what == lr::kNull ? SMI_CC_NULL : p.what == lr::kChimeric ? SMI_CC_CHIMERIA : p.what == lr::kNoUmi ? SMI_CC_NO_UMI : SMI_CC_MAPQV0]++;
            continue;
        }
        c[SMI_CC_VALID]++;
        auto put = [&](std::string_view s, std::vector<uint64_t> &off, std::vector<uint32_t> &len) {
            off.push_back(h->text.size());
            len.push_back((uint32_t)s.size());
            h->text.append(s);
        };
        put(lr::read_name(bam, recs[i]), h->name_off, h->name_len);
        put(lr::drop_minus1(p.bc), h->bc_off, h->bc_len);  // L83
        put(p.umi, h->umi_off, h->umi_len);
        put(p.cdna, h->cdna_off, h->cdna_len);
        h->de.push_back(p.de);
    }
    return SMI_OK;
}

extern "C" int smi_consensus_run(smi_consensus *h, float *kernel_ms) {
    if (!h) {
        set_error("smi_consensus_run: null argument");
        return SMI_ERR_INVALID;
    }
    if (kernel_ms) *kernel_ms = 0.f;
    if (h->ran) {
        set_error("smi_consensus_run: already run");
        return SMI_ERR_STATE;
    }
    h->ran = true;
    const char *T = h->text.data();
    auto sv = [&](const std::vector<uint64_t> &off, const std::vector<uint32_t> &len, size_t i) { return std::string_view(T + off[i], len[i]); };
    const size_t nk = h->de.size();
    // reads by name, in order of their first kept record (Longread.addRecord)
    std::unordered_map<std::string_view, int32_t> by_name;
    by_name.reserve(nk * 2 + 1);
    std::vector<int32_t> best, last, nrec;
    for (size_t i = 0; i < nk; i++) {
        auto it = by_name.emplace(sv(h->name_off, h->name_len, i), (int32_t)best.size());
        if (it.second) {
            best.push_back((int32_t)i);
            last.push_back((int32_t)i);
            nrec.push_back(1);
        } else {
            const int32_t r = it.first->second;
            if (float_less(h->de[i], h->de[best[r]])) best[r] = (int32_t)i;  // stable: the first of equal `de` stays
            last[r] = (int32_t)i;
            nrec[r]++;
        }
    }
    const size_t n_reads = best.size();
    int64_t *c = h->counts;
    c[SMI_CC_READS] = (int64_t)n_reads;
    c[SMI_CC_READS_MULTI] = 0;
    for (int32_t x : nrec) c[SMI_CC_READS_MULTI] += x > 1;
    // molecules keyed barcode:umi of the read's last kept record, in order of first appearance
    std::unordered_map<std::string, int32_t> by_key;
    by_key.reserve(n_reads + 1);
    std::vector<int32_t> mol_of(n_reads), mol_n;
    for (size_t r = 0; r < n_reads; r++) {
        std::string key(sv(h->bc_off, h->bc_len, last[r]));
        key += ':';
        key.append(sv(h->umi_off, h->umi_len, last[r]));
        auto it = by_key.emplace(std::move(key), (int32_t)mol_n.size());
        if (it.second) mol_n.push_back(0);
        mol_of[r] = it.first->second;
        mol_n[it.first->second]++;
    }
    const size_t n_mol = mol_n.size();
    c[SMI_CC_MOLECULES] = (int64_t)n_mol;
    std::vector<int64_t> mstart(n_mol + 1, 0);
    for (size_t m = 0; m < n_mol; m++) mstart[m + 1] = mstart[m] + mol_n[m];
    std::vector<int32_t> mreads(n_reads), fill(n_mol, 0);
    std::vector<int32_t> mol_last(n_mol);
    for (size_t r = 0; r < n_reads; r++) {
        const int32_t m = mol_of[r];
        mreads[mstart[m] + fill[m]++] = (int32_t)r;
        mol_last[m] = last[r];
    }
    // per molecule: reads by their best record's `de` (Float.compare, stable), the first MAXREADS
    const int max_reads = h->cfg.max_reads;
    std::vector<int32_t> nsel(n_mol);
    for (size_t m = 0; m < n_mol; m++) {
        auto b = mreads.begin() + mstart[m], e = mreads.begin() + mstart[m + 1];
        std::stable_sort(b, e, [&](int32_t x, int32_t y) { return float_less(h->de[best[x]], h->de[best[y]]); });
        nsel[m] = std::min<int32_t>(max_reads, mol_n[m]);
    }
    // K-POA for the molecules of 3 or more selected reads
    std::vector<int32_t> poa_mols;
    std::vector<uint64_t> roff{0};
    std::vector<int32_t> moff{0};
    std::string seqs;
    for (size_t m = 0; m < n_mol; m++) {
        if (nsel[m] < 3) continue;
        poa_mols.push_back((int32_t)m);
        for (int k = 0; k < nsel[m]; k++) {
            seqs.append(sv(h->cdna_off, h->cdna_len, best[mreads[mstart[m] + k]]));
            roff.push_back(seqs.size());
        }
        moff.push_back((int32_t)(roff.size() - 1));
    }
    c[SMI_CC_POA_MOLECULES] = (int64_t)poa_mols.size();
    std::vector<uint8_t> cons(std::max<size_t>(seqs.size(), 1));
    std::vector<uint32_t> same(cons.size());
    std::vector<int32_t> clen(poa_mols.size());
    if (!poa_mols.empty()) {
        int32_t bad = -1, n_rerun = 0;
        int64_t stats[SMI_POA_STATS];
        std::string why;
        const int rc = poa_batch(h->ctx, (const uint8_t *)seqs.data(), roff.data(), moff.data(), (int32_t)poa_mols.size(), (size_t)h->cfg.scratch_bytes,
                                 cons.data(), same.data(), clen.data(), kernel_ms, &n_rerun, &bad, &why, stats);
        if (rc) {
            if (bad >= 0) {  // the batch index back to the molecule's name
                const int32_t m = poa_mols[bad];
                set_error("ComputeConsensus: molecule " + std::string(sv(h->bc_off, h->bc_len, mol_last[m])) + "-" +
                          std::string(sv(h->umi_off, h->umi_len, mol_last[m])) + "-" + std::to_string(mol_n[m]) + " (" + why + ")");
            } else {
                set_error(std::string("ComputeConsensus: ") + smi_last_error());
            }
            return rc;
        }
        c[SMI_CC_POA_RERUN] = n_rerun;
        c[SMI_CC_POA_LAUNCHES] = stats[SMI_POA_STAT_LAUNCHES];
        c[SMI_CC_POA_SLOT_REUSE] = stats[SMI_POA_STAT_SLOT_REUSE];
    }
    // the FASTQ: @BC-UMI-n / cons / + / qv per molecule (Consensus.toFastq L233)
    std::string &fq = h->fastq;
    size_t k = 0;
    const char qmin = (char)(33 + h->cfg.min_ps);
    for (size_t m = 0; m < n_mol; m++) {
        fq += '@';
        fq.append(sv(h->bc_off, h->bc_len, mol_last[m]));
        fq += '-';
        fq.append(sv(h->umi_off, h->umi_len, mol_last[m]));
        fq += '-';
        fq += std::to_string(mol_n[m]);
        fq += '\n';
        if (nsel[m] < 3) {
            std::string_view s = sv(h->cdna_off, h->cdna_len, best[mreads[mstart[m]]]);
            if (nsel[m] == 2) {
                std::string_view s2 = sv(h->cdna_off, h->cdna_len, best[mreads[mstart[m] + 1]]);
                if (!(s.size() > s2.size())) s = s2;
            }
            fq.append(s);
            fq += "\n+\n";
            fq.append(s.size(), qmin);
        } else {
            const uint64_t o = roff[moff[k]];
            const int32_t L = clen[k];
            fq.append((const char *)cons.data() + o, L);
            fq += "\n+\n";
            for (int32_t i = 0; i < L; i++) fq += (char)qv_byte(same[o + i], (uint32_t)nsel[m], h->cfg.max_ps);
            k++;
        }
        fq += '\n';
    }
    return SMI_OK;
}

extern "C" int smi_consensus_fastq(const smi_consensus *h, uint8_t *out, size_t cap, size_t *n_out) {
    if (!h || !n_out) {
        set_error("smi_consensus_fastq: null argument");
        return SMI_ERR_INVALID;
    }
    return handle::get_text(h->fastq, out, cap, n_out);
}

extern "C" int smi_consensus_counts(const smi_consensus *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_consensus_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof(h->counts));
    return SMI_OK;
}
