// smi_collapse.hip -- `CollapseModel` (org/ipmc/sicelore/programs/CollapseModel.java:L151-193, the reference README's step 7, "Novel isoform
// discovery"): the unassigned (IT = undef) molecules of an ISOBAM are collapsed into novel isoforms per gene on the device, counted,
// filtered against the longer isoforms and the model, and classified; the refFlat model, the cell list, the record loader and the five
// output texts are host work.  The rules are DESIGN.md section 8h's; tests/collapsemodel.py implements the same ones.
//
// Host, in the reference's order:
//   model     UCSCRefFlatParser(File) L48-80 over TranscriptRecord.fromRefFlat L92-164: exons (start + 1, end), junctions (exon[i-1].end,
//             exon[i].start); a line whose exon bases sum to 0 is dropped; lines grouped by gene (column 0), in file order.  A line of fewer
//             than 11 fields, with a bad integer or a strand Strand.toStrand refuses ends the reference's parse silently: here it fails the
//             call naming the line.  select(gene, tx) (L120-131) = the last line of that gene with that transcript id.
//   cells     CellList.java L15-27: one barcode per line, every "-1" removed.
//   loader    UCSCRefFlatParser.loader L138-208 over LongreadRecord.fromSAMRecord(r, false) L71-184: a record is evidence of (IG, IT) when
//             it has a CELLTAG, is mapped, has mapq > 0, is not chimeric, RN >= RNMIN, its RAW CELLTAG value is in the cell list and its
//             GENETAG value is not null, "" or "undef".  The junction list is the literal walk of L138-171 (walk_junctions).  The evidence
//             order of a gene is reference-dictionary order (the loader queries sequence by sequence), then file order.
// K-COLLAPSE: one block per gene with an undef list (collapse L639-671 with isExactSameStructure L673-692), by rounds.
// K-COLSTAT: TranscriptRecord.initialize L357-399 per transcript, known and founder alike: evidence count, min txStart, max txEnd, the
//   last evidence record; distinct cells from (transcript << 32 | cell) codes, hipcub radix sort + run-length encoding; an exclusive scan
//   of the founder counts gives the Novel.<n> numbers (NOVELINDEX, L661).
// K-FILTER / K-CLASS: one wavefront per gene: filter L243-263 with isPartOfLonger L429-460 over the list the host sorted (Collections.sort
//   by TranscriptRecord.compareTo L85-90, stable), and noveltyDetector L379-427 for every novel it keeps.
// Host again: statistics L535-592 as counters, exportFiles L595-637 over printLegendTxt / printTxt / printRefflat / printGff
//   (TranscriptRecord.java L248-327): one renderer over the kept transcripts.
// The validator (validator L279-366 over BEDParser.java, smi_collapse_validate_*): the BED texts and both distances per transcript on the
//   host; K-JSUP: one lane per record of the short-read BAM, every alignment-block boundary looked up in a device table of the novel
//   junctions; then the validator's fields per transcript and the five texts again.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "smi_device.h"
#include "smi_handle.h"
#include "smi_internal.h"

namespace smi {
namespace {


constexpr const char *kWho = "CollapseModel";  // the program named when a device allocation fails

constexpr int kColThreads = 256;  // threads of one K-COLLAPSE block: 4 waves
constexpr int kColWaves = kColThreads / 64;
constexpr int kLdsJunc = 1024;    // junctions of a founder staged in LDS (8 KiB); a longer list is read from global memory
constexpr int kFcWaves = 4;       // waves per block of K-FILTER / K-CLASS

// isAllInclude(j1, j2) (L694-703): every junction of j1 isIn j2
__device__ __forceinline__ bool all_include(const int2 *__restrict__ j1, int n1, const int2 *__restrict__ j2, int n2, int d) {
    for (int i = 0; i < n1; i++)
        if (!is_in(j1[i], j2, n2, d)) return false;
    return true;
}

// K-COLLAPSE.  The reference's loop takes the undef records of a gene in order: record i joins the FIRST founder created before it for
// which isExactSameStructure holds, else it founds a transcript if it has a junction.  By rounds this is the same: round k takes the
// smallest record that is neither assigned nor mono-exonic -- every record in front of it has joined a founder of an earlier round or
// can never found, so it is exactly the reference's k-th founder, and founders arise in increasing record order -- and every unassigned
// record BEHIND it tests it.  A record still unassigned in round k matched none of the founders 0 .. k-1, so the founder it joins is
// the first that matches among those created before it; a founder behind the record is never tested against it (the reference has not
// created it yet when the record is looked at), and a mono-exonic record matches nothing (equal, non-zero junction counts).
// isExactSameStructure is one-sided, as in the reference: every FOUNDER junction isIn the record's junctions.
struct ColArgs {
    const int32_t *cg_off;   // n_cg + 1: undef records of collapse gene c, in evidence order
    const int32_t *u_j_off;  // n_u + 1: junctions of undef record u in uj
    const int2 *uj;
    int32_t delta, lds_junc;
    int32_t *u_founder;      // per undef record: ordinal of its founder within the gene, -1 none
    int32_t *cg_nf;          // per collapse gene: founders created
};

__global__ __launch_bounds__(kColThreads) void k_collapse(ColArgs a) {
    __shared__ int2 s_j[kLdsJunc];
    __shared__ int s_min[2][kColWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int u0 = a.cg_off[blockIdx.x], n = a.cg_off[blockIdx.x + 1] - u0;
    const int32_t *joff = a.u_j_off + u0;
    int32_t *founder = a.u_founder + u0;
    for (int i = tid; i < n; i += kColThreads) founder[i] = -1;
    __syncthreads();
    int nf = 0, cursor = 0, par = 0;
    while (cursor < n) {
        // the smallest unassigned multi-exon record from cursor on: a block reduction per chunk of kColThreads records
        int first = INT_MAX;
        for (int base = cursor; base < n && first == INT_MAX; base += kColThreads) {
            const int i = base + tid;
            const bool cand = i < n && founder[i] < 0 && joff[i + 1] > joff[i];
            const unsigned long long bal = __ballot(cand);
            if (lane == 0) s_min[par][wv] = bal ? base + wv * 64 + __ffsll((long long)bal) - 1 : INT_MAX;
            __syncthreads();
            for (int w = 0; w < kColWaves; w++) first = min(first, s_min[par][w]);
            par ^= 1;  // the next chunk writes the other half: no second barrier per chunk
        }
        if (first == INT_MAX) break;
        const int nj = joff[first + 1] - joff[first];
        const int2 *fj = a.uj + joff[first];
        const bool in_lds = nj <= a.lds_junc;
        if (in_lds)
            for (int k = tid; k < nj; k += kColThreads) s_j[k] = fj[k];
        if (tid == 0) founder[first] = nf;
        __syncthreads();
        const int2 *fl = in_lds ? s_j : fj;
        for (int r = first + 1 + tid; r < n; r += kColThreads) {
            if (founder[r] >= 0 || joff[r + 1] - joff[r] != nj) continue;
            const int2 *rl = a.uj + joff[r];
            bool ok = true;
            for (int k = 0; k < nj && ok; k++) ok = is_in(fl[k], rl, nj, a.delta);
            if (ok) founder[r] = nf;  // only this thread writes record r
        }
        nf++;
        cursor = first + 1;
        __syncthreads();
    }
    if (tid == 0) a.cg_nf[blockIdx.x] = nf;
}

// K-COLSTAT: per evidence record its transcript (a known slot, or n_slots + the founder's global number), the per-transcript statistics
// and the (transcript, cell) code
struct StatArgs {
    const int32_t *rec_slot;  // n_rec: known slot, or -1 = an undef record
    const int32_t *rec_u;     // n_rec: its index among the undef records
    const int32_t *u_cg;      // n_u: its collapse gene
    const int32_t *u_founder;
    const int32_t *cg_base;   // exclusive scan of cg_nf: Novel.<cg_base + ordinal + 1>
    const int32_t *tx_start, *tx_end, *cell;
    int32_t n_rec, n_slots;
    int32_t *t_count, *t_min, *t_max, *t_last;
    uint64_t *code;
};

__global__ void k_colstat(StatArgs a) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_rec) return;
    int t = a.rec_slot[r];
    if (t < 0) {
        const int u = a.rec_u[r], f = a.u_founder[u];
        t = f < 0 ? -1 : a.n_slots + a.cg_base[a.u_cg[u]] + f;
    }
    if (t < 0) {  // a mono-exonic undef record: evidence of nothing
        a.code[r] = ~0ull;
        return;
    }
    atomicAdd(&a.t_count[t], 1);
    atomicMin(&a.t_min[t], a.tx_start[r]);
    atomicMax(&a.t_max[t], a.tx_end[r]);
    atomicMax(&a.t_last[t], r);  // records are numbered in evidence order
    a.code[r] = (uint64_t)(uint32_t)t << 32 | (uint32_t)a.cell[r];
}

__global__ void k_colstat_init(int32_t *t_count, int32_t *t_min, int32_t *t_max, int32_t *t_last, int32_t *t_cells, int32_t n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    t_count[t] = 0;
    t_min[t] = INT_MAX;
    t_max[t] = INT_MIN;
    t_last[t] = -1;
    t_cells[t] = 0;
}

// one distinct (transcript, cell) code = one cell of that transcript
__global__ void k_colstat_cells(const uint64_t *__restrict__ ucode, const int64_t *__restrict__ n_run, int32_t *t_cells) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k >= *n_run || ucode[k] == ~0ull) return;
    atomicAdd(&t_cells[ucode[k] >> 32], 1);
}

// K-FILTER / K-CLASS
struct FcArgs {
    const int32_t *e_off;    // n_gene + 1: the gene's transcripts, sorted by exon count (descending, stable)
    const int32_t *e_j_off;  // per entry: its junctions in pool
    const int32_t *e_nj;
    const uint8_t *e_known;
    const int32_t *e_k_off;  // per entry: its junction kinds in kind (novels only)
    const int32_t *g_line0, *g_line1;  // per gene: its model lines [line0, line1), gene-major
    const int32_t *l_j_off;  // n_line + 1: junctions of model line l in pool (the model's junctions come first, gene-major)
    const int2 *pool;
    int32_t n_gene, delta;
    int32_t *keep;           // per entry
    int32_t *cat;            // per kept novel: 0 known junctions, 1 known splice sites, 2 a novel splice site
    uint8_t *kind;           // per junction of a kept novel, the same three
};

__global__ __launch_bounds__(64 * kFcWaves) void k_filter_class(FcArgs a) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kFcWaves + (threadIdx.x >> 6);
    if (g >= a.n_gene) return;
    const int e0 = a.e_off[g], e1 = a.e_off[g + 1];
    const int l0 = a.g_line0[g], nl = a.g_line1[g] - l0;
    const int2 *mj = a.pool + a.l_j_off[l0];  // every model junction of the gene
    const int nmj = a.l_j_off[l0 + nl] - a.l_j_off[l0];
    const int d = a.delta;
    for (int e = e0; e < e1; e++) {
        const int2 *ej = a.pool + a.e_j_off[e];
        const int nj = a.e_nj[e];
        bool keep = true;
        if (!a.e_known[e]) {
            // isPartOfLonger: the lanes take the transcripts kept so far, then the model lines of the gene
            const int nc = (e - e0) + nl;
            for (int c0 = 0; c0 < nc && keep; c0 += 64) {
                const int c = c0 + lane;
                bool hit = false;
                if (c < e - e0) {
                    if (a.keep[e0 + c])  // (c & 63) == lane: this lane stored that flag itself, below
                        hit = all_include(ej, nj, a.pool + a.e_j_off[e0 + c], a.e_nj[e0 + c], d);
                } else if (c < nc) {
                    const int l = l0 + (c - (e - e0));
                    hit = all_include(ej, nj, a.pool + a.l_j_off[l], a.l_j_off[l + 1] - a.l_j_off[l], d);
                }
                if (__any(hit)) keep = false;
            }
        }
        // keep is wave-uniform (__any).  The flag of entry e is stored by the lane that reads it back for the later entries (candidate c
        // goes to lane c & 63), so every flag a lane loads is one it stored itself: program order, no fence and no atomics
        if (lane == ((e - e0) & 63)) a.keep[e] = keep ? 1 : 0;
        if (keep && !a.e_known[e]) {
            // noveltyDetector: known junction (isIn with DELTA), else both ends exact members of the model's splice sites, else novel
            int worst = 0;
            for (int k = lane; k < nj; k += 64) {
                const int2 j = ej[k];
                int kd = 0;
                if (!is_in(j, mj, nmj, d)) {
                    bool sx = false, sy = false;
                    for (int i = 0; i < nmj; i++) {
                        sx |= mj[i].x == j.x || mj[i].y == j.x;
                        sy |= mj[i].x == j.y || mj[i].y == j.y;
                    }
                    kd = sx && sy ? 1 : 2;
                }
                a.kind[a.e_k_off[e] + k] = (uint8_t)kd;
                worst = max(worst, kd);
            }
            for (int o = 32; o > 0; o >>= 1) worst = max(worst, __shfl_xor(worst, o));
            if (lane == 0) a.cat[e] = worst;
        }
    }
}

// K-JSUP: the junction support of UCSCRefFlatParser.validator L321-345 for every novel junction at once.  One lane per record of SHORT: the
// alignment blocks of SAMRecord.getAlignmentBlocks (M / = / X, zero-length ones included; I / S move the read, D / N the reference, H / P
// nothing) are walked keeping the previous block's end, and every boundary (last base of the previous block, first base of the next,
// 1-based) that differs from the lane's previous one is looked up in the table of (SHORT reference id, donor, acceptor) keys: open
// addressing, linear probing, wrapping.  A hit is one atomic add whose result nobody reads.  The keys never change while the kernel runs,
// so they are read with plain loads; the counters live in an array of their own.  A record with flag 0x4 supports nothing.
__host__ __device__ __forceinline__ uint32_t jsup_hash(int32_t ref, int32_t donor, int32_t acceptor) {
    uint32_t h = (uint32_t)ref * 0x9E3779B1u ^ (uint32_t)donor * 0x85EBCA77u ^ (uint32_t)acceptor * 0xC2B2AE3Du;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    return h ^ h >> 12;
}

struct JsupArgs {
    const uint8_t *bam;
    const uint64_t *rec_off;    // n: offset of the record's block_size word
    int32_t n, n_ref;
    const uint8_t *ref_keys;    // n_ref: 1 = some key lies on this reference of SHORT
    const int4 *keys;           // mask + 1 slots: (reference, donor, acceptor, 0); reference -1 = empty
    uint32_t mask;
    uint32_t *count;            // mask + 1
    unsigned long long *boundaries;
};

__global__ __launch_bounds__(256) void k_jsup(JsupArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t looked = 0;
    if (i < a.n) {
        const uint8_t *r = a.bam + a.rec_off[i];
        int32_t ref, pos;
        uint32_t w;
        __builtin_memcpy(&ref, r + 4, 4);
        __builtin_memcpy(&pos, r + 8, 4);
        __builtin_memcpy(&w, r + 16, 4);  // n_cigar_op, flag
        const uint32_t n_op = w & 0xffff;
        if (n_op >= 2 && !(w >> 16 & 4) && (uint32_t)ref < (uint32_t)a.n_ref && a.ref_keys[ref]) {
            const uint8_t *cg = r + 36 + r[12];
            uint32_t at = (uint32_t)pos + 1;  // the reference base the next operation starts on (int arithmetic, as the reference's)
            uint32_t prev_end = 0, last_d = 0, last_a = 0;
            bool block = false, have_last = false;
            for (uint32_t k = 0; k < n_op; k++) {
                uint32_t c;
                __builtin_memcpy(&c, cg + 4 * k, 4);
                const uint32_t op = c & 15, len = c >> 4;
                if (op == 0 || op == 7 || op == 8) {
                    if (block && !(have_last && last_d == prev_end && last_a == at)) {
                        last_d = prev_end;
                        last_a = at;
                        have_last = true;
                        looked++;
                        uint32_t s = jsup_hash(ref, (int32_t)last_d, (int32_t)last_a) & a.mask;
                        for (uint32_t step = 0; step <= a.mask; step++) {
                            const int4 e = a.keys[s];
                            if (e.x < 0) break;
                            if (e.x == ref && e.y == (int32_t)last_d && e.z == (int32_t)last_a) {
                                atomicAdd(&a.count[s], 1u);
                                break;
                            }
                            s = (s + 1) & a.mask;
                        }
                    }
                    prev_end = at + len - 1;
                    block = true;
                    at += len;
                } else if (op == 2 || op == 3) {
                    at += len;
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) looked += __shfl_xor(looked, o);
    if ((threadIdx.x & 63) == 0 && looked) atomicAdd(a.boundaries, (unsigned long long)looked);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
using lr::drop_minus1;
using lr::jint;
using lr::jsplit;

struct Line {  // one refFlat line kept by the model
    std::string gene, tx;
    int32_t tx_start, tx_end, cds_start, cds_end;
    std::vector<int32_t> xs, xe;  // exon starts (as written, 0-based) and ends
};

struct Model {
    std::vector<Line> lines;  // gene-major: genes in order of their first line, lines of a gene in file order
    std::vector<std::string> genes;
    std::unordered_map<std::string, int32_t> gene_id;
    std::vector<int32_t> gene_line_off;  // n_gene + 1
    std::vector<int32_t> l_j_off{0};     // n_line + 1
    std::vector<int2> tj;
    std::unordered_map<std::string, int32_t> select;  // gene \t tx -> the last line
};

int parse_model(const char *text, size_t n, Model &M) {
    std::vector<Line> lines;
    std::vector<int32_t> line_gene;
    size_t b = 0;
    int64_t lineno = 0;
    handle::RefFlatLine R;
    std::string err;
    while (b < n) {
        size_t e = b;
        while (e < n && text[e] != '\n') e++;
        const int kind = handle::refflat_line("CollapseModel", std::string_view(text + b, e - b), ++lineno, true, R, err);
        b = e + 1;
        if (kind == handle::kLineBad) {
            set_error(err);
            return SMI_ERR_INVALID;
        }
        if (kind == handle::kLineDropped) continue;
        Line L{std::string(R.gene), std::string(R.tx), R.tx_start, R.tx_end, R.cds_start, R.cds_end, R.xs, R.xe};
        L.xe.resize(L.xs.size());
        auto git = M.gene_id.emplace(L.gene, (int32_t)M.genes.size());
        if (git.second) M.genes.push_back(L.gene);
        line_gene.push_back(git.first->second);
        lines.push_back(std::move(L));
    }
    std::vector<int32_t> ord(lines.size());
    for (size_t i = 0; i < ord.size(); i++) ord[i] = (int32_t)i;
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return line_gene[x] < line_gene[y]; });
    M.gene_line_off.assign(M.genes.size() + 1, 0);
    for (int32_t g : line_gene) M.gene_line_off[g + 1]++;
    for (size_t g = 0; g < M.genes.size(); g++) M.gene_line_off[g + 1] += M.gene_line_off[g];
    for (int32_t i : ord) {
        Line &L = lines[i];
        for (size_t k = 1; k < L.xs.size(); k++) M.tj.push_back(make_int2(L.xe[k - 1], L.xs[k] + 1));
        M.l_j_off.push_back((int32_t)M.tj.size());
        M.select[L.gene + "\t" + L.tx] = (int32_t)M.lines.size();  // the last line wins
        M.lines.push_back(std::move(L));
    }
    return SMI_OK;
}

// one transcript of the output, as exportFiles prints it
struct OutTx {
    int32_t gene;  // index into smi_collapse::genes
    std::string tname, chrom;
    bool neg, known;
    int32_t cat;  // of a novel: 0 known junctions, 1 known splice sites, 2 a novel splice site
    int32_t s0, s1, c0, c1, umis, cells;
    std::vector<int32_t> xs, xe;
    std::vector<int2> nov;  // novelJunctions
    // the validator's fields, TranscriptRecord's defaults (L46-52) until smi_collapse_validate_end sets them
    int32_t junction_reads = 0, dist_cage = 0, dist_polya = 0;
    bool v_junction = false, v_cage = false, v_polya = false, valid = false;
};

// BEDParser: per chromosome and strand the features' pp (start for +, end for -), sorted, the smallest line per equal pp
struct BedSide {
    std::vector<int32_t> pp, idx;
};
struct Bed {
    std::unordered_map<std::string, BedSide> side[2];  // + / -
    int64_t references = 0, entries = 0;
};

struct Validator {
    Bed cage, polya;
    int32_t cage_co = 50, polya_co = 50, junc_co = 1;
    std::vector<int4> keys;                     // the table as uploaded
    std::vector<int32_t> tx_k_off{0}, tx_slot;  // per output transcript: the slots of its novel junctions, -1 = chromosome not in SHORT
    std::vector<uint8_t> ref_keys;
    DevBuf<int4> d_keys{kWho};
    DevBuf<uint32_t> d_count{kWho};
    DevBuf<uint8_t> d_ref_keys{kWho};
    DevBuf<unsigned long long> d_bound{kWho};
    uint32_t mask = 0;
    int32_t n_ref = 0;
    float ms = 0.f;
    bool ended = false;
};

}  // namespace
}  // namespace smi

using namespace smi;

struct smi_collapse {
    smi_ctx *ctx = nullptr;
    smi_collapse_config cfg = {};
    lr::TagSet tags;
    Model M;
    std::unordered_map<std::string, int32_t> listed;  // the cell list
    std::vector<std::string> refs;
    // kept records in file order
    std::unordered_map<std::string, int32_t> gene_id, cell_id;
    std::vector<std::string> genes;
    std::vector<int32_t> r_gene, r_line, r_cell, r_ref, r_start, r_end, r_j_off{0};
    std::vector<uint8_t> r_neg;
    std::vector<int2> rj;
    int64_t counts[SMI_COLLAPSE_COUNTS] = {};
    std::string out[SMI_COLLAPSE_OUTPUTS];
    std::string error_read;
    int64_t error_record = -1;
    int64_t seen = 0;
    bool ran = false, failed = false;
    // K-COLLAPSE's input and result, kept for smi_collapse_host_loop
    std::vector<int32_t> k_cg_off, k_u_j_off, k_u_founder;
    std::vector<int2> k_uj;
    std::vector<OutTx> txs;  // what smi_collapse_run kept, in output order
    std::unique_ptr<Validator> val;
    int64_t vcounts[SMI_COLLAPSE_VALIDATE_COUNTS] = {};
};

namespace smi {
namespace {

void append_int(std::string &s, int64_t v) { s += std::to_string(v); }

// Float.parseFloat as BEDCodec L161 calls it, for the decimal forms: white space trimmed, a sign, "NaN", "Infinity", or digits with an
// optional point, an optional exponent and an optional f / F / d / D.  (A hexadecimal floating literal is taken as malformed here.)
bool java_float_ok(std::string_view s) {
    while (!s.empty() && (unsigned char)s.front() <= ' ') s.remove_prefix(1);
    while (!s.empty() && (unsigned char)s.back() <= ' ') s.remove_suffix(1);
    if (!s.empty() && (s[0] == '+' || s[0] == '-')) s.remove_prefix(1);
    if (s == "NaN" || s == "Infinity") return true;
    size_t i = 0, digits = 0;
    while (i < s.size() && s[i] >= '0' && s[i] <= '9') i++, digits++;
    if (i < s.size() && s[i] == '.') {
        i++;
        while (i < s.size() && s[i] >= '0' && s[i] <= '9') i++, digits++;
    }
    if (!digits) return false;
    if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
        i++;
        if (i < s.size() && (s[i] == '+' || s[i] == '-')) i++;
        size_t ed = 0;
        while (i < s.size() && s[i] >= '0' && s[i] <= '9') i++, ed++;
        if (!ed) return false;
    }
    if (i < s.size() && (s[i] == 'f' || s[i] == 'F' || s[i] == 'd' || s[i] == 'D')) i++;
    return i == s.size();
}

// BEDParser(File) L27-60 over BEDCodec(StartOffset.ZERO).decode, line by line as AsciiLineReader cuts them (\n, \r\n or \r)
int parse_bed(const char *text, size_t n, const char *what, Bed &B) {
    std::unordered_map<std::string, int> chroms;
    size_t b = 0;
    int64_t lineno = 0;
    int32_t idx = 0;
    while (b < n) {
        size_t e = b;
        while (e < n && text[e] != '\n' && text[e] != '\r') e++;
        const std::string_view line(text + b, e - b);
        if (e < n && text[e] == '\r' && e + 1 < n && text[e + 1] == '\n') e++;
        b = e + 1;
        lineno++;
        auto fail = [&](const std::string &why) {
            set_error(std::string("CollapseModel: ") + what + " line " + std::to_string(lineno) + ": " + why);
            return SMI_ERR_INVALID;
        };
        bool blank = true;
        for (char ch : line) blank &= (unsigned char)ch <= ' ';
        if (blank || line[0] == '#' || line.substr(0, 5) == "track" || line.substr(0, 7) == "browser") continue;
        std::vector<std::string_view> tk;  // Pattern "\t|( +)", split(line, -1)
        size_t t0 = 0;
        for (size_t i = 0; i < line.size();) {
            if (line[i] != '\t' && line[i] != ' ') {
                i++;
                continue;
            }
            tk.push_back(line.substr(t0, i - t0));
            if (line[i] == '\t') i++;
            else
                while (i < line.size() && line[i] == ' ') i++;
            t0 = i;
        }
        tk.push_back(line.substr(t0));
        if (tk.size() < 2) continue;
        int32_t start, end;
        if (!jint(tk[1], start)) return fail("the start is not an integer");
        end = start;
        if (tk.size() > 2 && !jint(tk[2], end)) return fail("the end is not an integer");
        if (std::abs((int64_t)start) > (1 << 30) || std::abs((int64_t)end) > (1 << 30)) return fail("a start or end beyond 2^30");
        int strand = -1;  // NONE
        const bool scored = tk.size() <= 4 || java_float_ok(tk[4]);  // a NumberFormatException returns the feature as it is (L163-168)
        if (scored) {
            if (tk.size() > 5) {
                std::string_view st = tk[5];
                while (!st.empty() && (unsigned char)st.front() <= ' ') st.remove_prefix(1);
                strand = st.empty() ? -1 : st[0] == '+' ? 0 : st[0] == '-' ? 1 : -1;
            }
            if (tk.size() > 8 && tk[8].find(',') != std::string_view::npos) {  // ParsingUtils.parseColor L369-374
                const auto rgb = jsplit(tk[8], ',');
                int32_t v[3];
                bool number = true;
                for (size_t k = 0; k < 3 && number; k++) {
                    if (k >= rgb.size()) return fail("a colour of fewer than three parts");
                    number = jint(rgb[k], v[k]);  // a NumberFormatException gives black
                }
                if (number && (v[0] < 0 || v[0] > 255 || v[1] < 0 || v[1] > 255 || v[2] < 0 || v[2] > 255))
                    return fail("a colour part outside 0 .. 255");
            }
            if (tk.size() > 11) {  // createExons L209-231
                int32_t x, count;
                if (!jint(tk[6], x) || !jint(tk[7], x)) return fail("thickStart or thickEnd is not an integer");
                if (!jint(tk[9], count) || count < 0) return fail("the block count is not a count");
                for (int c = 11; c >= 10; c--) {
                    const auto parts = jsplit(tk[c], ',');
                    for (int32_t k = 0; k < count; k++)
                        if ((size_t)k >= parts.size() || !jint(parts[k], x)) return fail("fewer block sizes or starts than blocks, or one that is no integer");
                }
            }
        }
        const std::string chr(tk[0]);
        chroms.emplace(chr, 0);
        if (strand >= 0) {
            BedSide &S = B.side[strand][chr];
            S.pp.push_back(strand ? end : start);
            S.idx.push_back(idx);
        }
        idx++;
    }
    B.references = (int64_t)chroms.size();
    B.entries = idx;
    for (auto &side : B.side)
        for (auto &kv : side) {
            BedSide &S = kv.second;
            std::vector<int32_t> ord(S.pp.size());
            for (size_t i = 0; i < ord.size(); i++) ord[i] = (int32_t)i;
            std::sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return S.pp[x] != S.pp[y] ? S.pp[x] < S.pp[y] : S.idx[x] < S.idx[y]; });
            BedSide T;
            for (int32_t o : ord)
                if (T.pp.empty() || T.pp.back() != S.pp[o]) {  // the smallest line of an equal pp
                    T.pp.push_back(S.pp[o]);
                    T.idx.push_back(S.idx[o]);
                }
            S = std::move(T);
        }
    return SMI_OK;
}

// getDistanceCage L68-91 = getDistancePolyA L97-119: the first feature in file order of the smallest |pos - pp|
int32_t bed_distance(const Bed &B, const std::string &chrom, bool neg, int32_t pos) {
    int64_t min = INT32_MAX, minabs = INT32_MAX;
    const auto it = B.side[neg].find(chrom);
    if (it != B.side[neg].end()) {
        const BedSide &S = it->second;
        const size_t r = std::lower_bound(S.pp.begin(), S.pp.end(), pos) - S.pp.begin();
        int32_t best = -1;
        for (size_t k = r ? r - 1 : r; k <= r && k < S.pp.size(); k++) {
            const int64_t d = (int64_t)pos - S.pp[k], ad = d < 0 ? -d : d;
            if (ad < minabs || (best >= 0 && ad == minabs && S.idx[k] < best)) {
                min = d;
                minabs = ad;
                best = S.idx[k];
            }
        }
    }
    return (int32_t)(neg ? min : -min);
}

// exportFiles L595-637 over printLegendTxt / printTxt / printRefflat / printGff (TranscriptRecord.java L248-327), and the valid set of
// statistics L568-576: the known transcripts and the novels with is_valid
void render(smi_collapse *h) {
    static const char *kSub[] = {"combination_of_known_junctions", "combination_of_known_splicesites", "at_least_one_novel_splicesite"};
    static const char *kCol[] = {"#9dd122", "#c594e1", "#e65802"};
    std::string &txt = h->out[SMI_COL_OUT_TXT], &flat = h->out[SMI_COL_OUT_REFFLAT], &flatv = h->out[SMI_COL_OUT_FINAL_REFFLAT];
    std::string &gff = h->out[SMI_COL_OUT_GFF], &gffv = h->out[SMI_COL_OUT_FINAL_GFF];
    for (std::string &o : h->out) o.clear();
    txt = "geneId\ttranscriptId\tchrom\tstrand\ttxStart\ttxEnd\texons\tUMIs\tCells\tcategorie\tsubcategorie\tnovelJunctions"
          "\tnovelJunctions_reads\tis_valid_allNovelJunctions\tdist_cage\tis_valid_cage\tdist_polya\tis_valid_polya\tis_valid\n";
    int64_t *v = h->vcounts;
    for (int k = SMI_CVAL_ISOFORMS; k <= SMI_CVAL_NSS_EV; k++) v[k] = 0;
    auto tf = [](bool b) { return b ? "true" : "false"; };
    std::string one_flat, one_gff;
    for (const OutTx &t : h->txs) {
        const std::string &gname = h->genes[t.gene];
        const char *strand = t.neg ? "-" : "+";
        const std::string categorie = t.known ? "full_splice_match" : t.cat == 2 ? "novel_not_in_catalog" : "novel_in_catalog";
        const std::string sub = t.known ? "gencode" : kSub[t.cat];
        const std::string color = t.known ? "#014e8e" : kCol[t.cat];
        std::string nov;
        for (const int2 &j : t.nov) nov += (nov.empty() ? "" : ",") + std::to_string(j.x) + "-" + std::to_string(j.y);
        if (nov.empty()) nov = "-";
        const std::string umis = std::to_string(t.umis), cells = std::to_string(t.cells);
        const std::string head = gname + "\t" + t.tname + "\t" + t.chrom + "\t" + strand + "\t" + std::to_string(t.s0) + "\t" + std::to_string(t.s1) + "\t";
        txt += head + std::to_string(t.xs.size()) + "\t" + umis + "\t" + cells + "\t" + categorie + "\t" + sub + "\t" + nov + "\t" +
               std::to_string(t.junction_reads) + "\t" + tf(t.v_junction) + "\t" + std::to_string(t.dist_cage) + "\t" + tf(t.v_cage) + "\t" +
               std::to_string(t.dist_polya) + "\t" + tf(t.v_polya) + "\t" + tf(t.valid) + "\n";
        one_flat = head + std::to_string(t.c0) + "\t" + std::to_string(t.c1) + "\t" + std::to_string(t.xs.size()) + "\t";
        for (int32_t x : t.xs) {
            append_int(one_flat, (int64_t)x - 1);
            one_flat += ',';
        }
        one_flat += '\t';
        for (int32_t x : t.xe) {
            append_int(one_flat, x);
            one_flat += ',';
        }
        one_flat += '\n';
        const std::string ids = "gene_id \"" + gname + "\"; transcript_id \"" + t.tname + "\";";
        one_gff = t.chrom + "\tsicelore\ttranscript\t" + std::to_string(t.s0) + "\t" + std::to_string(t.s1) + "\t.\t" + strand + "\t.\t" + ids +
                  " category \"" + categorie + "\"; subcategory \"" + sub + "\"; UMIs \"" + umis + "\"; Cells \"" + cells + "\"; novelJunctions \"" +
                  nov + "\"; supportingReads \"" + std::to_string(t.junction_reads) + "\"; CAGEdist \"" + std::to_string(t.dist_cage) +
                  "\"; POLYAdist \"" + std::to_string(t.dist_polya) + "\"; color \"" + color + "\";\n";
        for (size_t k = 0; k < t.xs.size(); k++)
            one_gff += t.chrom + "\tsicelore\texon\t" + std::to_string(t.xs[k]) + "\t" + std::to_string(t.xe[k]) + "\t.\t" + strand + "\t.\t" + ids + "\n";
        flat += one_flat;
        gff += one_gff;
        if (t.known || t.valid) {
            flatv += one_flat;
            gffv += one_gff;
            const int k = t.known ? SMI_CVAL_GENCODE : SMI_CVAL_CKJ + 2 * t.cat;
            v[SMI_CVAL_ISOFORMS]++;
            v[SMI_CVAL_EVIDENCES] += t.umis;
            v[k]++;
            v[k + 1] += t.umis;
        }
    }
}

}  // namespace
}  // namespace smi

extern "C" int smi_collapse_default_config(smi_collapse_config *cfg) {
    if (!cfg) {
        set_error("smi_collapse_default_config: null argument");
        return SMI_ERR_INVALID;
    }
    *cfg = {};
    std::memcpy(cfg->cell_tag, "BC", 3);
    std::memcpy(cfg->umi_tag, "U8", 3);
    std::memcpy(cfg->gene_tag, "IG", 3);
    std::memcpy(cfg->iso_tag, "IT", 3);
    std::memcpy(cfg->rn_tag, "RN", 3);
    cfg->max_clip = 150;
    cfg->delta = 2;
    cfg->min_evidence = 2;
    cfg->rn_min = 1;
    cfg->n_threads = 20;
    cfg->lds_junc = kLdsJunc;
    return SMI_OK;
}

extern "C" int smi_collapse_create(smi_ctx *ctx, const smi_collapse_config *cfg, const char *refflat, size_t n_refflat, const char *csv, size_t n_csv,
                                   smi_collapse **out) {
    if (!ctx || !cfg || !out || (n_refflat && !refflat) || (n_csv && !csv)) {
        set_error("smi_collapse_create: null argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    const char *tags[] = {cfg->cell_tag, cfg->umi_tag, cfg->gene_tag, cfg->iso_tag, cfg->rn_tag};
    const char *what[] = {"CELLTAG", "UMITAG", "GENETAG", "ISOFORMTAG", "RNTAG"};
    for (int i = 0; i < 5; i++)
        if (!valid_tag(tags[i])) {
            set_error(std::string(what[i]) + " must be two characters");
            return SMI_ERR_INVALID;
        }
    // (a DELTA below 0 is taken as the reference takes it: isIn never holds, so nothing joins, nothing is contained and no junction is known)
    if (cfg->lds_junc < 1 || cfg->lds_junc > kLdsJunc) {
        set_error("smi_collapse_config.lds_junc must be 1 .. " + std::to_string(kLdsJunc));
        return SMI_ERR_INVALID;
    }
    smi_collapse *h = new smi_collapse();
    h->ctx = ctx;
    h->cfg = *cfg;
    h->cfg.n_threads = std::max(1, std::min(cfg->n_threads, 256));
    h->tags.set(lr::kCell, cfg->cell_tag).set(lr::kUmi, cfg->umi_tag).set(lr::kGene, cfg->gene_tag).set(lr::kRn, cfg->rn_tag).set(lr::kIso, cfg->iso_tag);
    if (int rc = parse_model(refflat, n_refflat, h->M)) {
        delete h;
        return rc;
    }
    for (std::string &cell : handle::cell_list(csv, n_csv)) h->listed.emplace(std::move(cell), 0);
    h->counts[SMI_COL_CELLS] = (int64_t)h->listed.size();
    h->counts[SMI_COL_MODEL_GENES] = (int64_t)h->M.genes.size();
    h->counts[SMI_COL_MODEL_TRANSCRIPTS] = (int64_t)h->M.lines.size();
    *out = h;
    return SMI_OK;
}

extern "C" int smi_collapse_free(smi_collapse *h) {
    delete h;
    return SMI_OK;
}

extern "C" int smi_collapse_set_references(smi_collapse *h, const char *const *ref_names, int32_t n_refs) {
    if (!h || n_refs < 0 || (n_refs && !ref_names)) {
        set_error("smi_collapse_set_references: null argument");
        return SMI_ERR_INVALID;
    }
    h->refs.clear();
    for (int32_t i = 0; i < n_refs; i++) h->refs.emplace_back(ref_names[i] ? ref_names[i] : "");
    return SMI_OK;
}

extern "C" int smi_collapse_error_read(const smi_collapse *h, char *name, size_t cap, int64_t *record) {
    if (!h || !record || (cap && !name)) {
        set_error("smi_collapse_error_read: null argument");
        return SMI_ERR_INVALID;
    }
    return handle::error_read(h->error_read, h->error_record, name, cap, record);
}

extern "C" int smi_collapse_counts(const smi_collapse *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_collapse_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof h->counts);
    return SMI_OK;
}

extern "C" int smi_collapse_output(const smi_collapse *h, int32_t which, uint8_t *out, size_t cap, size_t *n_out) {
    if (!h || !n_out || which < 0 || which >= SMI_COLLAPSE_OUTPUTS) {
        set_error("smi_collapse_output: bad argument");
        return SMI_ERR_INVALID;
    }
    return handle::get_text(h->out[which], out, cap, n_out);
}

extern "C" int smi_collapse_add_segment(smi_collapse *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n) {
    if (!h || n < 0 || (n && (!bam || !recs))) {
        set_error("smi_collapse_add_segment: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->ran || h->failed) {
        set_error(h->ran ? "smi_collapse_add_segment: the model was already collapsed (smi_collapse_run)"
                         : "smi_collapse_add_segment: an earlier segment failed");
        return SMI_ERR_STATE;
    }
    const auto listed = [&](std::string_view bc) { return h->listed.count(std::string(bc)) != 0; };
    const lr::Segment seg = lr::read_segment("smi_collapse_add_segment", bam, n_bam, recs, n, h->cfg.n_threads,
                                             [&](const uint8_t *b, const smi_bam_record &r, lr::Record &out, std::string &err) {
                                                 lr::read_collapse(b, r, h->tags, h->cfg.max_clip, h->cfg.rn_min, listed, out, err);
                                             });
    if (!seg.refused.empty()) {
        set_error(seg.refused);
        return SMI_ERR_INVALID;
    }
    const lr::Records &parsed = seg.recs;
    auto fail = [&](int32_t i, const std::string &why) {
        h->failed = true;
        h->error_read = std::string(lr::read_name(bam, recs[i]));
        h->error_record = h->seen + i;
        set_error("CollapseModel: read " + h->error_read + ": " + why);
        return SMI_ERR_INVALID;
    };
    // the first failing record in file order is the one named: the lookups of the kept records are part of the same pass
    std::vector<int32_t> line(n, -1);
    for (int32_t i = 0; i < n; i++) {
        const lr::Record &p = parsed[i];
        if (i == seg.first_error) return fail(i, seg.error);
        if (p.what != lr::kKept || (p.has_it && p.it == "undef")) continue;
        auto it = p.has_it ? h->M.select.find(std::string(p.gene) + "\t" + std::string(p.it)) : h->M.select.end();
        if (it == h->M.select.end())  // refmodel.select gives null: the reference fails on it later (L196 or initialize)
            return fail(i, p.has_it ? "transcript " + std::string(p.it) + " of the ISOFORMTAG is no transcript of gene " + std::string(p.gene) + " in the REFFLAT"
                                    : "no ISOFORMTAG attribute");
        line[i] = it->second;
    }
    // records and junctions are numbered in int32 from here on (the offsets below, the kernels' indices, the hipcub calls): refuse what
    // does not fit where it accumulates, as mtx::matrix does for its codes
    size_t add_rec = 0, add_junc = 0;
    for (int32_t i = 0; i < n; i++)
        if (parsed[i].what == lr::kKept) {
            add_rec++;
            add_junc += parsed[i].junc.size();
        }
    if (h->r_gene.size() + add_rec > (size_t)INT32_MAX || h->rj.size() + add_junc > (size_t)INT32_MAX) {
        h->failed = true;
        set_error("CollapseModel: more than 2^31 - 1 evidence records or junctions in one run");
        return SMI_ERR_INVALID;
    }
    int64_t *c = h->counts;
    for (int32_t i = 0; i < n; i++) {
        const lr::Record &p = parsed[i];
        c[SMI_COL_RECORDS]++;
        if (p.what != lr::kKept) {
            c[p.what == lr::kNull ? SMI_COL_NULL : p.what == lr::kMapq0 ? SMI_COL_MAPQ0 : p.what == lr::kChimeric ? SMI_COL_CHIMERIC
              : p.what == lr::kLowRn ? SMI_COL_LOW_RN : p.what == lr::kNotListed ? SMI_COL_NOT_LISTED : SMI_COL_NO_GENE]++;
            continue;
        }
        c[SMI_COL_KEPT]++;
        auto git = h->gene_id.emplace(std::string(p.gene), (int32_t)h->genes.size());
        if (git.second) h->genes.emplace_back(p.gene);
        auto cit = h->cell_id.emplace(drop_minus1(p.bc), (int32_t)h->cell_id.size());
        h->r_gene.push_back(git.first->second);
        h->r_line.push_back(line[i]);
        h->r_cell.push_back(cit.first->second);
        h->r_ref.push_back(recs[i].ref_id);
        h->r_start.push_back(p.tx_start);
        h->r_end.push_back(p.tx_end);
        h->r_neg.push_back((recs[i].flag & 16) ? 1 : 0);
        h->rj.insert(h->rj.end(), p.junc.begin(), p.junc.end());
        h->r_j_off.push_back((int32_t)h->rj.size());
    }
    h->seen += n;
    return SMI_OK;
}

extern "C" int smi_collapse_run(smi_collapse *h, float *stage_ms) {
    if (!h) {
        set_error("smi_collapse_run: null argument");
        return SMI_ERR_INVALID;
    }
    float ms[SMI_COLLAPSE_STAGES] = {};
    if (stage_ms) std::memset(stage_ms, 0, sizeof(ms));
    if (h->ran || h->failed) {
        set_error(h->ran ? "smi_collapse_run: already run" : "smi_collapse_run: a segment failed");
        return SMI_ERR_STATE;
    }
    h->ran = true;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    const Model &M = h->M;
    int64_t *c = h->counts;
    const int32_t delta = h->cfg.delta;
    const size_t nk = h->r_gene.size();
    if (h->rj.size() + M.tj.size() > (size_t)INT32_MAX) {
        set_error("CollapseModel: more than 2^31 - 1 junctions in one run");
        return SMI_ERR_INVALID;
    }
    // genes in byte order of their name; evidence order = reference-dictionary order, then file order
    const int32_t nG = (int32_t)h->genes.size();
    std::vector<int32_t> gord(nG), grank(nG);
    for (int32_t i = 0; i < nG; i++) gord[i] = i;
    std::sort(gord.begin(), gord.end(), [&](int32_t x, int32_t y) { return h->genes[x] < h->genes[y]; });
    for (int32_t i = 0; i < nG; i++) grank[gord[i]] = i;
    std::vector<int32_t> ev(nk);
    for (size_t i = 0; i < nk; i++) ev[i] = (int32_t)i;
    std::stable_sort(ev.begin(), ev.end(), [&](int32_t x, int32_t y) { return h->r_ref[x] < h->r_ref[y]; });
    // per evidence record (numbered in evidence order): gene, known slot or undef
    std::vector<int32_t> e_gene(nk), rec_slot(nk, -1), rec_u(nk, -1), tx_start(nk), tx_end(nk), cell(nk);
    std::vector<std::vector<int32_t>> gene_slots(nG), gene_undef(nG);
    std::vector<int32_t> slot_line;
    std::unordered_map<uint64_t, int32_t> slot_of;
    for (size_t k = 0; k < nk; k++) {
        const int32_t i = ev[k], g = grank[h->r_gene[i]];
        e_gene[k] = g;
        tx_start[k] = h->r_start[i];
        tx_end[k] = h->r_end[i];
        cell[k] = h->r_cell[i];
        if (h->r_line[i] < 0) {
            gene_undef[g].push_back((int32_t)k);
        } else {
            auto it = slot_of.emplace((uint64_t)(uint32_t)g << 32 | (uint32_t)h->r_line[i], (int32_t)slot_line.size());
            if (it.second) {
                slot_line.push_back(h->r_line[i]);
                gene_slots[g].push_back(it.first->second);
            }
            rec_slot[k] = it.first->second;
        }
    }
    const int32_t n_slots = (int32_t)slot_line.size();
    // the undef lists, gene by gene
    std::vector<int32_t> cg_gene, cg_off{0}, u_rec, u_cg, u_j_off{0};
    std::vector<int2> uj;
    for (int32_t g = 0; g < nG; g++) {
        if (gene_undef[g].empty()) continue;
        for (int32_t k : gene_undef[g]) {
            rec_u[k] = (int32_t)u_rec.size();
            u_rec.push_back(k);
            u_cg.push_back((int32_t)cg_gene.size());
            const int32_t i = ev[k];
            uj.insert(uj.end(), h->rj.begin() + h->r_j_off[i], h->rj.begin() + h->r_j_off[i + 1]);
            u_j_off.push_back((int32_t)uj.size());
            c[SMI_COL_MONOEXON] += h->r_j_off[i + 1] == h->r_j_off[i];
            c[SMI_COL_LONG_LISTS] += h->r_j_off[i + 1] - h->r_j_off[i] > h->cfg.lds_junc;
        }
        cg_gene.push_back(g);
        cg_off.push_back((int32_t)u_rec.size());
        c[SMI_COL_MAX_UNDEF] = std::max<int64_t>(c[SMI_COL_MAX_UNDEF], (int64_t)gene_undef[g].size());
    }
    const int32_t nCG = (int32_t)cg_gene.size(), nU = (int32_t)u_rec.size();
    c[SMI_COL_GENES] = nG;
    c[SMI_COL_UNDEF_RECORDS] = nU;
    int rc = 0;
    Events evt;
    // K-COLLAPSE
    std::vector<int32_t> u_founder(nU, -1), cg_nf(nCG, 0), cg_base(nCG + 1, 0);
    DevBuf<int32_t> d_cgo{kWho}, d_ujo{kWho}, d_uf{kWho}, d_nf{kWho}, d_base{kWho};
    DevBuf<int2> d_uj{kWho};
    if ((rc = d_cgo.put(cg_off, s)) || (rc = d_ujo.put(u_j_off, s)) || (rc = d_uj.put(uj, s)) || (rc = d_uf.alloc(nU)) || (rc = d_nf.alloc(nCG + 1)) ||
        (rc = d_base.alloc(nCG + 1)))
        return rc;
    SMI_HIP(hipMemsetAsync(d_nf.p, 0, (size_t)(nCG + 1) * 4, s));
    if (nCG) {
        ColArgs a = {d_cgo.p, d_ujo.p, d_uj.p, delta, h->cfg.lds_junc, d_uf.p, d_nf.p};
        if ((rc = evt.begin(s))) return rc;
        hipLaunchKernelGGL(k_collapse, dim3((unsigned)nCG), dim3(kColThreads), 0, s, a);
        SMI_HIP(hipGetLastError());
        if ((rc = evt.end(s, &ms[0]))) return rc;
    }
    // K-COLSTAT: the scan of the founder counts (the Novel.<n> numbers), then the statistics per transcript
    {
        Scratch tmp{kWho};
        const auto scan = [&](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, d_nf.p, d_base.p, nCG + 1, s); };
        if ((rc = reserve(tmp, scan))) return rc;
        if ((rc = evt.begin(s))) return rc;
        if ((rc = run_reserved(tmp, scan))) return rc;
        if ((rc = evt.end(s, &ms[1]))) return rc;
        SMI_HIP(hipMemcpy(cg_base.data(), d_base.p, (size_t)(nCG + 1) * 4, hipMemcpyDeviceToHost));
        if (nCG) SMI_HIP(hipMemcpy(cg_nf.data(), d_nf.p, (size_t)nCG * 4, hipMemcpyDeviceToHost));
        if (nU) SMI_HIP(hipMemcpy(u_founder.data(), d_uf.p, (size_t)nU * 4, hipMemcpyDeviceToHost));
    }
    const int32_t n_founders = cg_base[nCG], nT = n_slots + n_founders;
    c[SMI_COL_FOUNDERS] = n_founders;
    for (int32_t x : cg_nf) c[SMI_COL_MAX_FOUNDERS] = std::max<int64_t>(c[SMI_COL_MAX_FOUNDERS], x);
    std::vector<int32_t> t_count(nT), t_min(nT), t_max(nT), t_last(nT), t_cells(nT);
    if (nk && nT) {
        DevBuf<int32_t> d_slot{kWho}, d_ru{kWho}, d_ucg{kWho}, d_ts{kWho}, d_te{kWho}, d_cell{kWho}, d_cnt{kWho}, d_min{kWho}, d_max{kWho}, d_last{kWho}, d_cells{kWho};
        DevBuf<uint64_t> d_code{kWho}, d_sorted{kWho}, d_unique{kWho};
        DevBuf<uint32_t> d_rl{kWho};
        DevBuf<int64_t> d_nrun{kWho};
        Scratch tmp{kWho};
        if ((rc = d_slot.put(rec_slot, s)) || (rc = d_ru.put(rec_u, s)) || (rc = d_ucg.put(u_cg, s)) || (rc = d_ts.put(tx_start, s)) ||
            (rc = d_te.put(tx_end, s)) || (rc = d_cell.put(cell, s)) || (rc = d_cnt.alloc(nT)) || (rc = d_min.alloc(nT)) || (rc = d_max.alloc(nT)) ||
            (rc = d_last.alloc(nT)) || (rc = d_cells.alloc(nT)) || (rc = d_code.alloc(nk)) || (rc = d_sorted.alloc(nk)) || (rc = d_unique.alloc(nk)) ||
            (rc = d_rl.alloc(nk)) || (rc = d_nrun.alloc(1)))
            return rc;
        const auto cells = sort_rle(s, d_code.p, d_sorted.p, d_unique.p, d_rl.p, d_nrun.p, (int)nk, 64);
        if ((rc = cells.reserve(tmp))) return rc;
        StatArgs a = {d_slot.p, d_ru.p, d_ucg.p, d_uf.p, d_base.p, d_ts.p, d_te.p, d_cell.p, (int32_t)nk, n_slots,
                      d_cnt.p, d_min.p, d_max.p, d_last.p, d_code.p};
        if ((rc = evt.begin(s))) return rc;
        hipLaunchKernelGGL(k_colstat_init, dim3((unsigned)((nT + 255) / 256)), dim3(256), 0, s, d_cnt.p, d_min.p, d_max.p, d_last.p, d_cells.p, nT);
        hipLaunchKernelGGL(k_colstat, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, a);
        SMI_HIP(hipGetLastError());
        if ((rc = cells.run_reserved(tmp))) return rc;
        hipLaunchKernelGGL(k_colstat_cells, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, d_unique.p, d_nrun.p, d_cells.p);
        SMI_HIP(hipGetLastError());
        if ((rc = evt.end(s, &ms[1]))) return rc;
        SMI_HIP(hipMemcpy(t_count.data(), d_cnt.p, (size_t)nT * 4, hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(t_min.data(), d_min.p, (size_t)nT * 4, hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(t_max.data(), d_max.p, (size_t)nT * 4, hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(t_last.data(), d_last.p, (size_t)nT * 4, hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(t_cells.data(), d_cells.p, (size_t)nT * 4, hipMemcpyDeviceToHost));
    }
    // the founding record of every founder: the first record of its ordinal
    std::vector<int32_t> f_u(n_founders, -1);
    for (int32_t u = 0; u < nU; u++)
        if (u_founder[u] >= 0) {
            int32_t &f = f_u[cg_base[u_cg[u]] + u_founder[u]];
            if (f < 0) f = u;
        }
    // per gene: the known transcripts in order of their first evidence, then the founders of MINEVIDENCE records in creation order
    // (collapser L211-230); Collections.sort by exon count, descending and stable (filter L247)
    struct Entry {
        int32_t t, nex;  // transcript (slot, or n_slots + founder), exons
    };
    std::vector<int32_t> e_off{0}, e_t, e_j_off, e_nj, e_k_off, g_line0(nG, 0), g_line1(nG, 0);
    std::vector<uint8_t> e_known;
    const int32_t n_mj = (int32_t)M.tj.size();
    int32_t n_kind = 0;
    {
        std::vector<int32_t> cg_of(nG, -1);
        for (int32_t q = 0; q < nCG; q++) cg_of[cg_gene[q]] = q;
        std::vector<Entry> lst;
        for (int32_t g = 0; g < nG; g++) {
            lst.clear();
            for (int32_t sl : gene_slots[g]) lst.push_back({sl, (int32_t)M.lines[slot_line[sl]].xs.size()});
            if (cg_of[g] >= 0)
                for (int32_t f = cg_base[cg_of[g]]; f < cg_base[cg_of[g] + 1]; f++)
                    if (t_count[n_slots + f] >= h->cfg.min_evidence) {
                        lst.push_back({n_slots + f, u_j_off[f_u[f] + 1] - u_j_off[f_u[f]] + 1});
                        c[SMI_COL_NOVEL_EVIDENCED]++;
                    }
            std::stable_sort(lst.begin(), lst.end(), [](const Entry &x, const Entry &y) { return x.nex > y.nex; });
            for (const Entry &e : lst) {
                const bool known = e.t < n_slots;
                e_t.push_back(e.t);
                e_known.push_back(known);
                if (known) {
                    e_j_off.push_back(M.l_j_off[slot_line[e.t]]);
                    e_nj.push_back(M.l_j_off[slot_line[e.t] + 1] - M.l_j_off[slot_line[e.t]]);
                    e_k_off.push_back(0);
                } else {
                    const int32_t u = f_u[e.t - n_slots];
                    e_j_off.push_back(n_mj + u_j_off[u]);
                    e_nj.push_back(u_j_off[u + 1] - u_j_off[u]);
                    e_k_off.push_back(n_kind);
                    n_kind += e_nj.back();
                }
            }
            e_off.push_back((int32_t)e_t.size());
            auto mit = M.gene_id.find(h->genes[gord[g]]);
            if (mit != M.gene_id.end()) {
                g_line0[g] = M.gene_line_off[mit->second];
                g_line1[g] = M.gene_line_off[mit->second + 1];
            }
        }
    }
    const int32_t nE = (int32_t)e_t.size();
    std::vector<int32_t> keep(nE, 0), cat(nE, 0);
    std::vector<uint8_t> kind(n_kind, 0);
    if (nE) {
        std::vector<int2> pool(M.tj);
        pool.insert(pool.end(), uj.begin(), uj.end());
        DevBuf<int32_t> d_eo{kWho}, d_ejo{kWho}, d_enj{kWho}, d_eko{kWho}, d_l0{kWho}, d_l1{kWho}, d_ljo{kWho}, d_keep{kWho}, d_cat{kWho};
        DevBuf<uint8_t> d_ek{kWho}, d_kind{kWho};
        DevBuf<int2> d_pool{kWho};
        if ((rc = d_eo.put(e_off, s)) || (rc = d_ejo.put(e_j_off, s)) || (rc = d_enj.put(e_nj, s)) || (rc = d_ek.put(e_known, s)) ||
            (rc = d_eko.put(e_k_off, s)) || (rc = d_l0.put(g_line0, s)) || (rc = d_l1.put(g_line1, s)) || (rc = d_ljo.put(M.l_j_off, s)) ||
            (rc = d_pool.put(pool, s)) || (rc = d_keep.alloc(nE)) || (rc = d_cat.alloc(nE)) || (rc = d_kind.alloc(n_kind)))
            return rc;
        SMI_HIP(hipMemsetAsync(d_keep.p, 0, (size_t)nE * 4, s));
        SMI_HIP(hipMemsetAsync(d_cat.p, 0, (size_t)nE * 4, s));
        FcArgs a = {d_eo.p, d_ejo.p, d_enj.p, d_ek.p, d_eko.p, d_l0.p, d_l1.p, d_ljo.p, d_pool.p, nG, delta, d_keep.p, d_cat.p, d_kind.p};
        if ((rc = evt.begin(s))) return rc;
        hipLaunchKernelGGL(k_filter_class, dim3((unsigned)((nG + kFcWaves - 1) / kFcWaves)), dim3(64 * kFcWaves), 0, s, a);
        SMI_HIP(hipGetLastError());
        if ((rc = evt.end(s, &ms[2]))) return rc;
        SMI_HIP(hipMemcpy(keep.data(), d_keep.p, (size_t)nE * 4, hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(cat.data(), d_cat.p, (size_t)nE * 4, hipMemcpyDeviceToHost));
        if (n_kind) SMI_HIP(hipMemcpy(kind.data(), d_kind.p, (size_t)n_kind, hipMemcpyDeviceToHost));
    }
    // the transcripts exportFiles prints: genes in byte order, a gene's transcripts in the filter's order
    for (int32_t g = 0; g < nG; g++) {
        for (int32_t e = e_off[g]; e < e_off[g + 1]; e++) {
            if (!keep[e]) {
                c[SMI_COL_NOVEL_FILTERED]++;
                continue;
            }
            const int32_t t = e_t[e];
            const int32_t last = ev[t_last[t]];  // chromosome and strand of the LAST evidence record, for known transcripts too
            OutTx o;
            o.gene = gord[g];
            o.known = e_known[e];
            o.chrom = h->r_ref[last] < (int32_t)h->refs.size() ? h->refs[h->r_ref[last]] : std::string("*");
            o.neg = h->r_neg[last];
            o.cat = 0;
            if (o.known) {
                const Line &L = M.lines[slot_line[t]];
                o.tname = L.tx;
                o.s0 = L.tx_start;
                o.s1 = L.tx_end;
                o.c0 = L.cds_start;
                o.c1 = L.cds_end;
                for (size_t k = 0; k < L.xs.size(); k++) {
                    o.xs.push_back(L.xs[k] + 1);
                    o.xe.push_back(L.xe[k]);
                }
                c[SMI_COL_GENCODE]++;
                c[SMI_COL_GENCODE_EV] += t_count[t];
            } else {
                const int32_t f = t - n_slots, u = f_u[f];
                o.tname = "Novel." + std::to_string(f + 1);
                o.cat = cat[e];
                o.s0 = o.c0 = t_min[t];
                o.s1 = o.c1 = t_max[t];
                const int2 *j = uj.data() + u_j_off[u];
                const int32_t nj = e_nj[e];
                o.xs.push_back(o.s0);
                for (int32_t k = 0; k < nj; k++) {
                    o.xe.push_back(j[k].x);
                    o.xs.push_back(j[k].y);
                    if (kind[e_k_off[e] + k]) o.nov.push_back(j[k]);
                }
                o.xe.push_back(o.s1);
                c[SMI_COL_CKJ + 2 * cat[e]]++;
                c[SMI_COL_CKJ_EV + 2 * cat[e]] += t_count[t];
            }
            c[SMI_COL_ISOFORMS]++;
            c[SMI_COL_EVIDENCES] += t_count[t];
            o.umis = t_count[t];
            o.cells = t_cells[t];
            h->txs.push_back(std::move(o));
        }
    }
    render(h);  // no novel is valid without the validator (smi_collapse_validate_*)
    h->k_cg_off = std::move(cg_off);
    h->k_u_j_off = std::move(u_j_off);
    h->k_u_founder = std::move(u_founder);
    h->k_uj = std::move(uj);
    if (stage_ms) std::memcpy(stage_ms, ms, sizeof(ms));
    return SMI_OK;
}

extern "C" int smi_collapse_validate_begin(smi_collapse *h, const char *cage, size_t n_cage, const char *polya, size_t n_polya,
                                           const char *const *short_ref_names, int32_t n_refs, int32_t cage_co, int32_t polya_co, int32_t junc_co,
                                           int32_t table_log2) {
    if (!h || (n_cage && !cage) || (n_polya && !polya) || n_refs < 0 || (n_refs && !short_ref_names)) {
        set_error("smi_collapse_validate_begin: null argument");
        return SMI_ERR_INVALID;
    }
    if (!h->ran || h->failed || h->val) {
        set_error(h->val ? "smi_collapse_validate_begin: already called" : "smi_collapse_validate_begin: smi_collapse_run comes first");
        return SMI_ERR_STATE;
    }
    if (table_log2 < 0 || table_log2 > 30) {
        set_error("smi_collapse_validate_begin: table_log2 must be 0 .. 30");
        return SMI_ERR_INVALID;
    }
    auto V = std::make_unique<Validator>();
    V->cage_co = cage_co;
    V->polya_co = polya_co;
    V->junc_co = junc_co;
    int rc;
    if ((rc = parse_bed(cage, n_cage, "CAGE", V->cage)) || (rc = parse_bed(polya, n_polya, "POLYA", V->polya))) return rc;
    std::unordered_map<std::string, int32_t> short_id;
    for (int32_t i = 0; i < n_refs; i++) short_id.emplace(short_ref_names[i] ? short_ref_names[i] : "", i);
    V->n_ref = n_refs;
    V->ref_keys.assign(std::max(n_refs, 1), 0);
    // validator L299-308: the distances of every transcript, known ones included; L310-316: its keys
    struct Key {
        int32_t ref, donor, acceptor;
    };
    std::vector<Key> keys;
    std::unordered_map<std::string, int32_t> key_id;
    std::vector<int32_t> tx_key;
    for (OutTx &t : h->txs) {
        t.dist_cage = bed_distance(V->cage, t.chrom, t.neg, t.neg ? t.s1 : t.s0);
        t.dist_polya = bed_distance(V->polya, t.chrom, t.neg, t.neg ? t.s0 : t.s1);
        t.v_cage = std::abs((int64_t)t.dist_cage) <= cage_co;
        t.v_polya = std::abs((int64_t)t.dist_polya) <= polya_co;
        const auto sit = short_id.find(t.chrom);
        for (const int2 &j : t.nov) {
            if (sit == short_id.end()) {
                tx_key.push_back(-1);
                continue;
            }
            const Key k{sit->second, j.x, j.y};
            const auto kit = key_id.emplace(std::string((const char *)&k, sizeof k), (int32_t)keys.size());
            if (kit.second) keys.push_back(k);
            tx_key.push_back(kit.first->second);
        }
        V->tx_k_off.push_back((int32_t)tx_key.size());
    }
    uint64_t size = 16;
    if (table_log2) size = 1ull << table_log2;
    else
        while (size < 2 * (uint64_t)keys.size()) size <<= 1;
    if (size < keys.size() || size > (1ull << 30)) {
        set_error("CollapseModel: a junction table of " + std::to_string(size) + " slots does not hold the " + std::to_string(keys.size()) +
                  " novel junctions to validate");
        return SMI_ERR_INVALID;
    }
    V->mask = (uint32_t)(size - 1);
    V->keys.assign(size, make_int4(-1, 0, 0, 0));
    std::vector<int32_t> key_slot(keys.size());
    for (size_t i = 0; i < keys.size(); i++) {
        uint32_t s = jsup_hash(keys[i].ref, keys[i].donor, keys[i].acceptor) & V->mask;
        while (V->keys[s].x >= 0) s = (s + 1) & V->mask;  // (the table holds every key: a free slot exists)
        V->keys[s] = make_int4(keys[i].ref, keys[i].donor, keys[i].acceptor, 0);
        key_slot[i] = (int32_t)s;
        V->ref_keys[keys[i].ref] = 1;
    }
    for (int32_t k : tx_key) V->tx_slot.push_back(k < 0 ? -1 : key_slot[k]);
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    if ((rc = V->d_keys.put(V->keys, s)) || (rc = V->d_ref_keys.put(V->ref_keys, s)) || (rc = V->d_count.alloc(size)) || (rc = V->d_bound.alloc(1)))
        return rc;
    SMI_HIP(hipMemsetAsync(V->d_count.p, 0, size * sizeof(uint32_t), s));
    SMI_HIP(hipMemsetAsync(V->d_bound.p, 0, sizeof(unsigned long long), s));
    SMI_HIP(hipStreamSynchronize(s));
    int64_t *v = h->vcounts;
    v[SMI_CVAL_JUNCTION_KEYS] = (int64_t)keys.size();
    v[SMI_CVAL_TABLE_SLOTS] = (int64_t)size;
    v[SMI_CVAL_CAGE_REFERENCES] = V->cage.references;
    v[SMI_CVAL_CAGE_ENTRIES] = V->cage.entries;
    v[SMI_CVAL_POLYA_REFERENCES] = V->polya.references;
    v[SMI_CVAL_POLYA_ENTRIES] = V->polya.entries;
    h->val = std::move(V);
    return SMI_OK;
}

extern "C" int smi_collapse_validate_segment(smi_collapse *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n) {
    if (!h || n < 0 || (n && (!bam || !recs))) {
        set_error("smi_collapse_validate_segment: null argument");
        return SMI_ERR_INVALID;
    }
    if (!h->val || h->val->ended) {
        set_error("smi_collapse_validate_segment: between smi_collapse_validate_begin and smi_collapse_validate_end");
        return SMI_ERR_STATE;
    }
    Validator &V = *h->val;
    // K-JSUP reads the fixed part and the CIGAR from the segment's own bytes: both inside the segment, by those bytes
    std::vector<uint64_t> off(n);
    for (int32_t i = 0; i < n; i++) {
        const uint64_t o = recs[i].rec_off;
        bool ok = o <= n_bam && n_bam - o >= 36;
        if (ok) {
            uint16_t n_op;
            std::memcpy(&n_op, bam + o + 16, 2);
            ok = n_bam - o - 36 >= (uint64_t)bam[o + 12] + 4ull * n_op;
        }
        if (!ok) {
            set_error("smi_collapse_validate_segment: record " + std::to_string(i) + " lies outside the segment");
            return SMI_ERR_INVALID;
        }
        off[i] = o;
    }
    h->vcounts[SMI_CVAL_SHORT_RECORDS] += n;
    if (n == 0 || h->vcounts[SMI_CVAL_JUNCTION_KEYS] == 0) return SMI_OK;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    DevBuf<uint8_t> d_bam{kWho};
    DevBuf<uint64_t> d_off{kWho};
    int rc;
    if ((rc = d_bam.alloc(n_bam)) || (rc = d_off.put(off, s))) return rc;
    SMI_HIP(hipMemcpyAsync(d_bam.p, bam, n_bam, hipMemcpyHostToDevice, s));
    JsupArgs a = {d_bam.p, d_off.p, n, V.n_ref, V.d_ref_keys.p, V.d_keys.p, V.mask, V.d_count.p, V.d_bound.p};
    Events evt;
    if ((rc = evt.begin(s))) return rc;
    hipLaunchKernelGGL(k_jsup, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    SMI_HIP(hipGetLastError());
    if ((rc = evt.end(s, &V.ms))) return rc;
    return SMI_OK;
}

extern "C" int smi_collapse_validate_end(smi_collapse *h, float *stage_ms) {
    if (!h) {
        set_error("smi_collapse_validate_end: null argument");
        return SMI_ERR_INVALID;
    }
    if (stage_ms) *stage_ms = 0.f;
    if (!h->val || h->val->ended) {
        set_error(h->val ? "smi_collapse_validate_end: already called" : "smi_collapse_validate_end: smi_collapse_validate_begin comes first");
        return SMI_ERR_STATE;
    }
    Validator &V = *h->val;
    V.ended = true;
    SMI_HIP(hipSetDevice(h->ctx->device));
    std::vector<uint32_t> count(V.keys.size());
    unsigned long long bound = 0;
    SMI_HIP(hipMemcpy(count.data(), V.d_count.p, count.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(&bound, V.d_bound.p, sizeof bound, hipMemcpyDeviceToHost));
    h->vcounts[SMI_CVAL_SHORT_BOUNDARIES] = (int64_t)bound;
    for (uint32_t x : count) h->vcounts[SMI_CVAL_JUNCTION_HITS] += x;
    for (size_t i = 0; i < h->txs.size(); i++) {  // validator L310-361
        OutTx &t = h->txs[i];
        uint32_t total = 0;
        bool ok = true;
        for (int32_t k = V.tx_k_off[i]; k < V.tx_k_off[i + 1]; k++) {
            const int32_t support = V.tx_slot[k] < 0 ? 0 : (int32_t)count[V.tx_slot[k]];
            total += (uint32_t)support;
            ok &= support >= V.junc_co;
        }
        t.junction_reads = (int32_t)total;
        t.v_junction = ok;
        t.valid = t.v_cage && t.v_polya && ok;
    }
    render(h);
    if (stage_ms) *stage_ms = V.ms;
    return SMI_OK;
}

extern "C" int smi_collapse_validate_counts(const smi_collapse *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_collapse_validate_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->vcounts, sizeof h->vcounts);
    return SMI_OK;
}

// collapse() L639-671 as the reference runs it: one thread, record by record against the founders so far
extern "C" int smi_collapse_host_loop(const smi_collapse *h, double *seconds, int64_t *mismatches) {
    if (!h || !seconds || !mismatches) {
        set_error("smi_collapse_host_loop: null argument");
        return SMI_ERR_INVALID;
    }
    if (!h->ran) {
        set_error("smi_collapse_host_loop: smi_collapse_run comes first");
        return SMI_ERR_STATE;
    }
    const int32_t d = h->cfg.delta;
    const int2 *uj = h->k_uj.data();
    const int32_t *joff = h->k_u_j_off.data();
    auto is_in = [&](int2 j, const int2 *l, int n) {
        bool b = false;
        for (int i = 0; i < n; i++)
            if (std::abs(l[i].x - j.x) <= d && std::abs(l[i].y - j.y) <= d) b = true;
        return b;
    };
    std::vector<int32_t> got(h->k_u_founder.size(), -1), founders;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t g = 0; g + 1 < h->k_cg_off.size(); g++) {
        founders.clear();
        for (int32_t u = h->k_cg_off[g]; u < h->k_cg_off[g + 1]; u++) {
            const int nj = joff[u + 1] - joff[u];
            bool seen = false;
            for (size_t f = 0; f < founders.size(); f++) {
                const int32_t fu = founders[f];
                bool same = nj > 0 && joff[fu + 1] - joff[fu] == nj;
                for (int k = 0; same && k < nj; k++) same = is_in(uj[joff[fu] + k], uj + joff[u], nj);
                if (same && !seen) {
                    got[u] = (int32_t)f;
                    seen = true;
                }
            }
            if (!seen && nj > 0) {
                got[u] = (int32_t)founders.size();
                founders.push_back(u);
            }
        }
    }
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *mismatches = 0;
    for (size_t u = 0; u < got.size(); u++) *mismatches += got[u] != h->k_u_founder[u];
    return SMI_OK;
}
