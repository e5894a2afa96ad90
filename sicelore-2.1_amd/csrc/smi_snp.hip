// smi_snp.hip -- `SNPMatrix` (org/ipmc/sicelore/programs/SNPMatrix.java:L72-216): per-cell SNP / editing-site matrices of a molecule BAM.
// K-SNP finds, for every record, the site lines it overlaps on its strand and the read base and quality under each of their positions;
// K-MTX (smi_mtx.h) counts the distinct UMIs per (row, cell) and renders the dense matrix.  The rules are DESIGN.md section 8e's;
// tests/snpmodel.py implements the same ones.
//
// Host: the SNP file (L100-120: lines `chromosome,position[|position...],strand,name` up to the first empty line; a chromosome outside the
//   BAM's dictionary skips the line; positions sorted ascending, their text kept as written), the cell list (CellList: "-1" removed),
//   the checks of what the reference swallows in mid-run (see smi_snp_add_segment), the interning of UMIs and rows, the metrics and
//   molinfos texts.
// K-SNP: one wavefront per record, two launches (count, hipcub exclusive scan, write).  A first pass over the CIGAR sums the reference
//   length; the lines of the record's chromosome are sorted by first position with a running maximum of last position, so the
//   candidates [first <= end, running max >= start] come from two binary searches; lanes test 64 candidates at a time (query(..,
//   contained = false) L121 and the strand test L126).  Per candidate line the CIGAR is walked 64 operations per round: a wave prefix
//   sum gives every operation its reference and read start, and the lane whose M / = / X operation covers a requested position resolves
//   it (SAMRecord.getReadPositionAtReferencePosition, L140), reads the quality byte and the 4-bit base; positions are taken in ascending
//   order, so one walk serves any number of them.  The record's attributes (CELLTAG, UMITAG, RNTAG; the types the reference casts) are
//   walked once by lane 0 and the barcode, "-1" removed, is looked up in a hash table of the cell list (FNV-1a, linear probing, bytes
//   compared).  Output per pair: record, line, cell or -1, rn, status (hit / lowRN / lowQV, L165-180), and per position base and quality.
// K-MTX: (row, cell, UMI id) triples of the hits of listed cells: two stable hipcub radix sorts (by UMI, then by row and cell), a flag
//   kernel and a select drop the repeats; the run lengths of what is left are the distinct UMIs (Matrix.addMolecule L88-105).
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "smi_handle.h"
#include "smi_internal.h"
#include "smi_mtx.h"

namespace smi {
namespace {

using lr::jint;
using lr::jsplit;

constexpr int kSnpWaves = 4;  // waves per block of K-SNP
constexpr uint64_t kCellBasis = 1469598103934665603ull;  // where the FNV-1a walk over a barcode starts: the host's cell table and find_cell

enum : uint32_t { kHit = 0, kLowRn = 1, kLowQv = 2, kStatusMask = 0xff, kPairNoQual = 1u << 8, kPairNoUmi = 1u << 9 };
enum : uint8_t { kRecConsidered = 1, kRecBadAux = 2, kRecBadType = 4, kRecNotNull = 8 };

constexpr const char *kWho = "SNPMatrix";  // the program named when a device allocation fails

struct SnpPair {
    int32_t rec, line, cell, rn;  // record of the segment, kept line (file order), cell id or -1 (not in the list)
    uint32_t status, npos;
    uint64_t byte_off;  // bases at bq[byte_off ..+ npos), qualities behind them
};

struct SnpArgs {
    const uint8_t *bam;
    const smi_bam_record *recs;
    int32_t n, n_ref;
    const int32_t *ref_off;                               // n_ref + 1: lines of reference r, sorted by first position
    const int32_t *l_first, *l_last, *l_runmax, *l_id;    // l_runmax: the largest last position up to this line
    const uint8_t *l_neg;
    const int32_t *l_pos_off, *pos;                       // CSR: the positions of a line, ascending
    const uint8_t *cell_text;
    const uint32_t *cell_off;
    const int32_t *cell_tab;                              // open addressing, -1 = empty
    uint32_t tab_mask;
    uint16_t tag_cell, tag_umi, tag_gene, tag_rn;
    int32_t min_rn, min_qv;
    uint64_t *n_pairs, *n_bytes;                          // COUNT: per record; WRITE: their exclusive scans
    uint8_t *rec_flags;
    SnpPair *pairs;
    uint8_t *bq;
};

struct AuxInfo {
    uint32_t flags;  // kRecBadAux / kRecBadType
    int32_t rn, cell;
    bool has_cell, has_umi;
};

// the barcode with every "-1" removed (String.replace, left to right) against the cell list
__device__ int32_t find_cell(const SnpArgs &a, const uint8_t *s, uint32_t n) {
    uint64_t h = kCellBasis;
    for (uint32_t i = 0; i < n; i++) {
        if (s[i] == '-' && i + 1 < n && s[i + 1] == '1') {
            i++;
            continue;
        }
        h = fnv1a_add(h, s[i]);
    }
    for (uint32_t slot = (uint32_t)h & a.tab_mask;; slot = (slot + 1) & a.tab_mask) {
        const int32_t id = a.cell_tab[slot];
        if (id < 0) return -1;
        const uint8_t *c = a.cell_text + a.cell_off[id];
        const uint32_t cn = a.cell_off[id + 1] - a.cell_off[id];
        uint32_t j = 0;
        bool same = true;
        for (uint32_t i = 0; i < n && same; i++) {
            if (s[i] == '-' && i + 1 < n && s[i + 1] == '1') {
                i++;
                continue;
            }
            same = j < cn && c[j] == s[i];
            j++;
        }
        if (same && j == cn) return id;
    }
}

// LongreadRecord.fromSAMRecord L75-95 over the BAM attribute bytes: the last value of a tag counts; GENETAG, CELLTAG, UMITAG are cast to
// String, de (else df) to Float, RNTAG to Integer
__device__ AuxInfo scan_aux(const SnpArgs &a, const smi_bam_record &r) {
    AuxInfo o = {0, 1, -1, false, false};
    const uint8_t *p = a.bam + r.aux_off, *end = p + r.aux_len;
    const uint8_t *cell = nullptr, *rn = nullptr;
    uint32_t cell_n = 0;
    uint8_t t_cell = 0, t_umi = 0, t_gene = 0, t_rn = 0, t_de = 0, t_df = 0;
    while (p < end) {
        size_t n;
        if (lr::aux_size(p, end, &n)) {
            o.flags |= kRecBadAux;
            break;
        }
        const uint16_t tag = (uint16_t)(p[0] | p[1] << 8);
        const uint8_t t = p[2];
        if (tag == a.tag_cell) {
            t_cell = t;
            cell = p + 3;
            cell_n = (uint32_t)n - 4;
        }
        if (tag == a.tag_umi) t_umi = t;
        if (tag == a.tag_gene) t_gene = t;
        if (tag == a.tag_rn) {
            t_rn = t;
            rn = p + 3;
        }
        if (tag == (uint16_t)('d' | 'e' << 8)) t_de = t;
        if (tag == (uint16_t)('d' | 'f' << 8)) t_df = t;
        p += n;
    }
    if (o.flags) return o;
    if ((t_cell && t_cell != 'Z') || (t_umi && t_umi != 'Z') || (t_gene && t_gene != 'Z') || (t_de ? t_de != 'f' : (t_df && t_df != 'f')))
        o.flags |= kRecBadType;
    if (t_rn) {
        switch (t_rn) {
            case 'c': o.rn = (int8_t)rn[0]; break;
            case 'C': o.rn = rn[0]; break;
            case 's': o.rn = (int16_t)(rn[0] | rn[1] << 8); break;
            case 'S': o.rn = rn[0] | rn[1] << 8; break;
            case 'i': case 'I': {
                const uint32_t v = ld_u32(rn);
                if (t_rn == 'I' && v > 0x7fffffffu) o.flags |= kRecBadType;
                o.rn = (int32_t)v;
                break;
            }
            default: o.flags |= kRecBadType;
        }
    }
    if (o.flags) return o;
    o.has_cell = t_cell != 0;
    o.has_umi = t_umi != 0;
    if (o.has_cell) o.cell = find_cell(a, cell, cell_n);
    return o;
}

// the positions pp[0 .. P) (ascending) of one line against the record's CIGAR: true when every position lies in an M / = / X operation
// at a read offset below the read length (L138-146: min > 0 and readLength > max).  *min_q: the smallest quality (at most 100, L149).
// EMIT: base (complemented on the reverse strand, 0 = the empty string of complementBase) and quality per position at bq / bq + P.
template <bool EMIT>
__device__ bool resolve(const SnpArgs &a, const smi_bam_record &r, int lane, const int32_t *__restrict__ pp, int P, int64_t start, bool neg,
                        int *min_q, uint8_t *bq) {
    int pi = 0, myq = 100;
    bool fail = false;
    int64_t ref_base = start, read_base = 1;  // of the round's first operation; read offsets are 1-based and count S, not H
    for (int k0 = 0; k0 < (int)r.n_cigar && !fail && pi < P; k0 += 64) {
        const int k = k0 + lane;
        uint32_t c = 0;
        if (k < (int)r.n_cigar) c = ld_u32(a.bam + r.cigar_off + 4ull * k);
        const uint32_t op = c & 15;
        const int64_t len = c >> 4;
        const bool is_m = op == 0 || op == 7 || op == 8;
        const int64_t rl = (is_m || op == 2 || op == 3) ? len : 0, ql = (is_m || op == 1 || op == 4) ? len : 0;
        const int64_t ir = wave_incl_sum(rl, lane), iq = wave_incl_sum(ql, lane);
        const int64_t rs = ref_base + ir - rl, qs = read_base + iq - ql;
        const int64_t round_end = ref_base + (int64_t)__shfl((long long)ir, 63);
        while (pi < P) {
            const int64_t p = pp[pi];
            if (p >= round_end) break;
            const int64_t rp = p - rs + qs;
            const bool ok = is_m && p >= rs && p < rs + len && rp < (int64_t)r.l_seq;
            if (!__ballot(ok)) {
                fail = true;
                break;
            }
            if (ok) {
                const uint8_t q = a.bam[r.qual_off + (uint64_t)(rp - 1)];
                myq = min(myq, (int)q);
                if (EMIT) {
                    const uint8_t two = a.bam[r.seq_off + (uint64_t)((rp - 1) >> 1)];
                    const uint32_t code = ((rp - 1) & 1) ? (two & 15u) : (uint32_t)(two >> 4);
                    uint8_t b = (uint8_t)"=ACMGRSVTWYHKDBN"[code];
                    if (neg) b = b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : 0;
                    bq[pi] = b;
                    bq[P + pi] = q;
                }
            }
            pi++;
        }
        ref_base = round_end;
        read_base += (int64_t)__shfl((long long)iq, 63);
    }
    if (pi < P) fail = true;
    for (int o = 32; o > 0; o >>= 1) myq = min(myq, __shfl_xor(myq, o));
    *min_q = myq;
    return !fail;
}

template <bool WRITE>
__global__ __launch_bounds__(64 * kSnpWaves) void k_snp(SnpArgs a) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kSnpWaves + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const smi_bam_record r = a.recs[i];
    uint64_t np = 0, nb = 0;
    uint32_t rflags = 0;
    const uint64_t pair_at = WRITE ? a.n_pairs[i] : 0, byte_at = WRITE ? a.n_bytes[i] : 0;
    if (r.ref_id >= 0 && r.ref_id < a.n_ref && a.ref_off[r.ref_id + 1] > a.ref_off[r.ref_id]) {
        const int l0 = a.ref_off[r.ref_id], l1 = a.ref_off[r.ref_id + 1];
        int64_t reflen = 0;
        for (int k = lane; k < (int)r.n_cigar; k += 64) {
            const uint8_t *q = a.bam + r.cigar_off + 4ull * k;
            const uint32_t c = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24, op = c & 15;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += c >> 4;
        }
        for (int o = 32; o > 0; o >>= 1) reflen += (int64_t)__shfl_xor((long long)reflen, o);
        const int64_t start = (int64_t)r.pos + 1, end = start + reflen - 1;
        const bool neg = (r.flag & 16) != 0;
        int lo = l0, hi = l1;  // ub: the first line whose first position lies behind the alignment
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)a.l_first[mid] <= end) lo = mid + 1;
            else hi = mid;
        }
        const int ub = lo;
        lo = l0, hi = ub;  // lb: the first line up to which some last position reaches the alignment
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)a.l_runmax[mid] < start) lo = mid + 1;
            else hi = mid;
        }
        bool aux_done = false, notnull = false, has_umi = false;
        int32_t rn = 1, cell = -1;
        for (int base = lo; base < ub; base += 64) {
            const int li = base + lane;
            const bool cand = li < ub && (int64_t)a.l_last[li] >= start && (a.l_neg[li] != 0) == neg;
            unsigned long long bal = __ballot(cand);
            while (bal) {
                const int L = base + (__ffsll((long long)bal) - 1);
                bal &= bal - 1;
                if (!aux_done) {  // the record reaches fromSAMRecord (L128): its attributes, once
                    aux_done = true;
                    AuxInfo x = {0, 1, -1, false, false};
                    if (lane == 0) x = scan_aux(a, r);
                    const uint32_t fl = __shfl(x.flags, 0);
                    rn = __shfl(x.rn, 0);
                    cell = __shfl(x.cell, 0);
                    has_umi = __shfl((int)x.has_umi, 0) != 0;
                    notnull = fl == 0 && __shfl((int)x.has_cell, 0) != 0 && !(r.flag & 4);  // L80: no barcode or unmapped -> null
                    rflags = kRecConsidered | fl | (notnull ? kRecNotNull : 0);
                }
                if (!notnull) continue;
                const int P = a.l_pos_off[L + 1] - a.l_pos_off[L];
                const int32_t *pp = a.pos + a.l_pos_off[L];
                int min_q = 100;
                if (!resolve<false>(a, r, lane, pp, P, start, neg, &min_q, nullptr)) continue;
                if (WRITE) {
                    resolve<true>(a, r, lane, pp, P, start, neg, &min_q, a.bq + byte_at + nb);
                    if (lane == 0) {
                        uint32_t st = rn < a.min_rn ? kLowRn : min_q < a.min_qv ? kLowQv : kHit;  // L165-180
                        if (r.l_seq > 0 && a.bam[r.qual_off] == 0xff) st |= kPairNoQual;
                        if ((st & kStatusMask) == kHit && cell >= 0 && !has_umi) st |= kPairNoUmi;
                        SnpPair o;
                        o.rec = i;
                        o.line = a.l_id[L];
                        o.cell = cell;
                        o.rn = rn;
                        o.status = st;
                        o.npos = (uint32_t)P;
                        o.byte_off = byte_at + nb;
                        a.pairs[pair_at + np] = o;
                    }
                }
                np++;
                nb += 2ull * (uint64_t)P;
            }
        }
    }
    if (!WRITE && lane == 0) {
        a.n_pairs[i] = np;
        a.n_bytes[i] = nb;
        a.rec_flags[i] = (uint8_t)rflags;
    }
}

// first[i]: (code, umi) i differs from the entry before it in the sorted order
__global__ void k_snp_first(const uint64_t *__restrict__ code, const uint32_t *__restrict__ umi, int64_t n, uint8_t *__restrict__ first) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    first[i] = i == 0 || code[i] != code[i - 1] || umi[i] != umi[i - 1];
}

struct Line {
    int32_t ref = -1;
    bool neg = false;
    std::string chrom, gene, pos_text;  // pos_text: the positions as written, joined by '|'
    std::vector<int32_t> arr;           // ascending
    int64_t cnt[3] = {0, 0, 0};         // hits, lowRN, lowQV
};

struct Hit {
    int32_t line, cell, umi, rn;
    uint64_t bq_off;  // bases, then qualities, in h->hit_bq
};

}  // namespace
}  // namespace smi

using namespace smi;

struct smi_snp {
    smi_ctx *ctx = nullptr;
    smi_snp_config cfg = {};
    std::vector<Line> lines;       // kept lines in file order
    std::vector<int32_t> text_line;  // per line read from the file: its index in `lines`, or -1 (chromosome not in the BAM)
    std::vector<std::string> cells;  // byte order
    int32_t n_ref = 0;
    // device tables
    DevBuf<int32_t> d_ref_off{kWho}, d_first{kWho}, d_last{kWho}, d_runmax{kWho}, d_id{kWho}, d_pos_off{kWho}, d_pos{kWho}, d_tab{kWho};
    DevBuf<uint8_t> d_neg{kWho}, d_cell_text{kWho};
    DevBuf<uint32_t> d_cell_off{kWho};
    uint32_t tab_mask = 0;
    // hits of listed cells, in record order
    std::vector<Hit> hits;
    std::vector<uint8_t> hit_bq;
    std::vector<std::string> umis;
    std::unordered_map<std::string, int32_t> umi_id;
    int64_t counts[SMI_SNP_COUNTS] = {};
    float ms[SMI_SNP_STAGES] = {};
    std::string out[SMI_SNP_OUTPUTS];
    bool ran = false;
};

extern "C" int smi_snp_default_config(smi_snp_config *cfg) {
    if (!cfg) {
        set_error("smi_snp_default_config: null argument");
        return SMI_ERR_INVALID;
    }
    *cfg = {};
    std::memcpy(cfg->cell_tag, "BC", 3);
    std::memcpy(cfg->umi_tag, "U8", 3);
    std::memcpy(cfg->gene_tag, "GE", 3);
    std::memcpy(cfg->rn_tag, "RN", 3);
    cfg->max_clip = 150;
    cfg->min_rn = 0;
    cfg->min_qv = 0;
    cfg->n_threads = 20;
    cfg->budget_bytes = 0;
    return SMI_OK;
}

extern "C" int smi_snp_create(smi_ctx *ctx, const smi_snp_config *cfg, const char *snp, size_t n_snp, const char *csv, size_t n_csv,
                              const char *const *ref_names, int32_t n_refs, smi_snp **out) {
    if (!ctx || !cfg || !out || (n_snp && !snp) || (n_csv && !csv) || n_refs < 0 || (n_refs && !ref_names)) {
        set_error("smi_snp_create: null argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    const char *tags[] = {cfg->cell_tag, cfg->umi_tag, cfg->gene_tag, cfg->rn_tag};
    const char *what[] = {"CELLTAG", "UMITAG", "GENETAG", "RNTAG"};
    for (int i = 0; i < 4; i++)
        if (!valid_tag(tags[i])) {
            set_error(std::string(what[i]) + " must be two characters");
            return SMI_ERR_INVALID;
        }
    std::unique_ptr<smi_snp> h(new smi_snp());
    h->ctx = ctx;
    h->cfg = *cfg;
    h->cfg.n_threads = std::max(1, std::min(cfg->n_threads, 256));
    h->n_ref = n_refs;
    std::unordered_map<std::string, int32_t> dict;  // SAMSequenceDictionary.getSequence(name)
    for (int32_t i = 0; i < n_refs; i++) dict.emplace(ref_names[i] ? ref_names[i] : "", i);
    // the SNP file: readLine (\n, \r\n or \r) until the end or the first empty line (L101-102)
    size_t b = 0;
    int64_t lineno = 0;
    while (b < n_snp) {
        size_t e = b;
        while (e < n_snp && snp[e] != '\n' && snp[e] != '\r') e++;
        const std::string_view line(snp + b, e - b);
        if (e < n_snp && snp[e] == '\r' && e + 1 < n_snp && snp[e + 1] == '\n') e++;
        b = e + 1;
        lineno++;
        if (line.empty()) break;
        auto fail = [&](const std::string &why) {
            set_error("SNPMatrix: SNP line " + std::to_string(lineno) + " (" + std::string(line) + "): " + why);
            return SMI_ERR_INVALID;
        };
        const auto tok = jsplit(line, ',');
        if (tok.empty()) return fail("no fields");
        const auto it = dict.find(std::string(tok[0]));
        if (it == dict.end()) {  // L107: skipped without a word (the header line goes this way)
            h->text_line.push_back(-1);
            continue;
        }
        if (tok.size() < 4) return fail("has " + std::to_string(tok.size()) + " fields, 4 are needed (chromosome,position,strand,name)");
        Line L;
        L.ref = it->second;
        L.chrom = std::string(tok[0]);
        L.neg = tok[2] == "-";
        L.gene = std::string(tok[3]);
        std::vector<std::string_view> pos{tok[1]};
        if (tok[1].find('|') != std::string_view::npos) pos = jsplit(tok[1], '|');  // L116-118
        if (pos.empty()) return fail("no position");
        for (size_t k = 0; k < pos.size(); k++) {
            int32_t v;
            if (!jint(pos[k], v)) return fail("position '" + std::string(pos[k]) + "' is not an integer");
            L.arr.push_back(v);
            if (k) L.pos_text += '|';
            L.pos_text.append(pos[k]);
        }
        std::sort(L.arr.begin(), L.arr.end());
        h->text_line.push_back((int32_t)h->lines.size());
        h->lines.push_back(std::move(L));
    }
    // CellList: every line with "-1" removed
    std::vector<std::string> cells = handle::cell_list(csv, n_csv);
    std::sort(cells.begin(), cells.end());
    cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
    h->cells = std::move(cells);
    h->counts[SMI_SNP_LINES] = (int64_t)h->lines.size();
    h->counts[SMI_SNP_CELLS] = (int64_t)h->cells.size();
    // device tables: lines per reference by (first, last position), the cell hash table
    const size_t nl = h->lines.size();
    std::vector<int32_t> ord(nl);
    for (size_t i = 0; i < nl; i++) ord[i] = (int32_t)i;
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) {
        const Line &p = h->lines[x], &q = h->lines[y];
        return p.ref != q.ref ? p.ref < q.ref : p.arr.front() < q.arr.front();
    });
    std::vector<int32_t> ref_off(n_refs + 1, 0), first(nl), last(nl), runmax(nl), id(nl), pos_off{0}, pos;
    std::vector<uint8_t> neg(nl);
    for (size_t k = 0; k < nl; k++) {
        const Line &L = h->lines[ord[k]];
        ref_off[L.ref + 1]++;
        first[k] = L.arr.front();
        last[k] = L.arr.back();
        runmax[k] = k && h->lines[ord[k - 1]].ref == L.ref ? std::max(runmax[k - 1], last[k]) : last[k];
        id[k] = ord[k];
        neg[k] = L.neg;
        pos.insert(pos.end(), L.arr.begin(), L.arr.end());
        pos_off.push_back((int32_t)pos.size());
    }
    for (int32_t r = 0; r < n_refs; r++) ref_off[r + 1] += ref_off[r];
    std::vector<uint8_t> cell_text;
    std::vector<uint32_t> cell_off{0};
    uint32_t tsize = 2;
    while (tsize < 2 * h->cells.size() + 2) tsize <<= 1;
    std::vector<int32_t> tab(tsize, -1);
    h->tab_mask = tsize - 1;
    for (size_t i = 0; i < h->cells.size(); i++) {
        const std::string &c = h->cells[i];
        cell_text.insert(cell_text.end(), c.begin(), c.end());
        cell_off.push_back((uint32_t)cell_text.size());
        uint64_t x = kCellBasis;
        for (unsigned char ch : c) x = fnv1a_add(x, ch);
        uint32_t slot = (uint32_t)x & h->tab_mask;
        while (tab[slot] >= 0) slot = (slot + 1) & h->tab_mask;
        tab[slot] = (int32_t)i;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) {
        set_error("smi_snp_create: hipSetDevice failed");
        return SMI_ERR_HIP;
    }
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = h->d_ref_off.put(ref_off, s)) || (rc = h->d_first.put(first, s)) || (rc = h->d_last.put(last, s)) || (rc = h->d_runmax.put(runmax, s)) ||
        (rc = h->d_id.put(id, s)) || (rc = h->d_neg.put(neg, s)) || (rc = h->d_pos_off.put(pos_off, s)) || (rc = h->d_pos.put(pos, s)) ||
        (rc = h->d_cell_text.put(cell_text, s)) || (rc = h->d_cell_off.put(cell_off, s)) || (rc = h->d_tab.put(tab, s)))
        return rc;
    SMI_HIP(hipStreamSynchronize(s));
    *out = h.release();
    return SMI_OK;
}

extern "C" int smi_snp_free(smi_snp *h) {
    delete h;
    return SMI_OK;
}

extern "C" int smi_snp_add_segment(smi_snp *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n) {
    if (!h || n < 0 || (n && (!bam || !recs))) {
        set_error("smi_snp_add_segment: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->ran) {
        set_error("smi_snp_add_segment: the matrix was already built (smi_snp_run)");
        return SMI_ERR_STATE;
    }
    for (int32_t i = 0; i < n; i++) {  // K-SNP reads the CIGAR, the bases, the qualities and the attributes: all inside the segment
        const smi_bam_record &r = recs[i];
        if (r.l_seq < 0 || r.name_off + r.l_read_name > n_bam || r.cigar_off + 4ull * r.n_cigar > n_bam ||
            r.seq_off + ((uint64_t)r.l_seq + 1) / 2 > n_bam || r.qual_off + (uint64_t)r.l_seq > n_bam || r.aux_off + r.aux_len > n_bam) {
            set_error("smi_snp_add_segment: record " + std::to_string(i) + " lies outside the segment");
            return SMI_ERR_INVALID;
        }
    }
    h->counts[SMI_SNP_RECORDS] += n;
    if (n == 0 || h->lines.empty()) return SMI_OK;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    DevBuf<uint8_t> d_bam{kWho}, d_flags{kWho}, d_bq{kWho};
    Scratch tmp{kWho};
    DevBuf<smi_bam_record> d_recs{kWho};
    DevBuf<uint64_t> d_np{kWho}, d_nb{kWho}, d_op{kWho}, d_ob{kWho};
    DevBuf<SnpPair> d_pairs{kWho};
    int rc;
    if ((rc = d_bam.alloc(n_bam)) || (rc = d_recs.alloc(n)) || (rc = d_flags.alloc(n)) || (rc = d_np.alloc(n + 1)) || (rc = d_nb.alloc(n + 1)) ||
        (rc = d_op.alloc(n + 1)) || (rc = d_ob.alloc(n + 1)))
        return rc;
    SMI_HIP(hipMemcpyAsync(d_bam.p, bam, n_bam, hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemcpyAsync(d_recs.p, recs, (size_t)n * sizeof(smi_bam_record), hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemsetAsync(d_np.p, 0, (n + 1) * sizeof(uint64_t), s));
    SMI_HIP(hipMemsetAsync(d_nb.p, 0, (n + 1) * sizeof(uint64_t), s));
    SnpArgs a = {};
    a.bam = d_bam.p;
    a.recs = d_recs.p;
    a.n = n;
    a.n_ref = h->n_ref;
    a.ref_off = h->d_ref_off.p;
    a.l_first = h->d_first.p;
    a.l_last = h->d_last.p;
    a.l_runmax = h->d_runmax.p;
    a.l_id = h->d_id.p;
    a.l_neg = h->d_neg.p;
    a.l_pos_off = h->d_pos_off.p;
    a.pos = h->d_pos.p;
    a.cell_text = h->d_cell_text.p;
    a.cell_off = h->d_cell_off.p;
    a.cell_tab = h->d_tab.p;
    a.tab_mask = h->tab_mask;
    a.tag_cell = lr::tag16(h->cfg.cell_tag);
    a.tag_umi = lr::tag16(h->cfg.umi_tag);
    a.tag_gene = lr::tag16(h->cfg.gene_tag);
    a.tag_rn = lr::tag16(h->cfg.rn_tag);
    a.min_rn = h->cfg.min_rn;
    a.min_qv = h->cfg.min_qv;
    a.n_pairs = d_np.p;
    a.n_bytes = d_nb.p;
    a.rec_flags = d_flags.p;
    const unsigned grid = (unsigned)((n + kSnpWaves - 1) / kSnpWaves);
    Events ev;
    if ((rc = ev.begin(s))) return rc;
    hipLaunchKernelGGL(k_snp<false>, dim3(grid), dim3(64 * kSnpWaves), 0, s, a);
    SMI_HIP(hipGetLastError());
    const auto sum = [&](uint64_t *in, uint64_t *out) {  // (the iterator types of the renderer's scan: one set of scan kernels in this file)
        return run(tmp, [=](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, in, out, n + 1, s); });
    };
    if ((rc = sum(d_np.p, d_op.p)) || (rc = sum(d_nb.p, d_ob.p))) return rc;
    if ((rc = ev.end(s, &h->ms[0]))) return rc;
    uint64_t n_pairs = 0, n_bytes = 0;
    SMI_HIP(hipMemcpy(&n_pairs, d_op.p + n, sizeof(uint64_t), hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(&n_bytes, d_ob.p + n, sizeof(uint64_t), hipMemcpyDeviceToHost));
    std::vector<uint8_t> flags(n), bq(n_bytes);
    std::vector<SnpPair> pairs(n_pairs);
    SMI_HIP(hipMemcpy(flags.data(), d_flags.p, n, hipMemcpyDeviceToHost));
    if (n_pairs) {
        if ((rc = d_pairs.alloc(n_pairs)) || (rc = d_bq.alloc(n_bytes))) return rc;
        a.n_pairs = d_op.p;
        a.n_bytes = d_ob.p;
        a.pairs = d_pairs.p;
        a.bq = d_bq.p;
        if ((rc = ev.begin(s))) return rc;
        hipLaunchKernelGGL(k_snp<true>, dim3(grid), dim3(64 * kSnpWaves), 0, s, a);
        SMI_HIP(hipGetLastError());
        if ((rc = ev.end(s, &h->ms[0]))) return rc;
        SMI_HIP(hipMemcpy(pairs.data(), d_pairs.p, n_pairs * sizeof(SnpPair), hipMemcpyDeviceToHost));
        if (n_bytes) SMI_HIP(hipMemcpy(bq.data(), d_bq.p, n_bytes, hipMemcpyDeviceToHost));
    }
    auto name_of = [&](int32_t i) { return std::string((const char *)bam + recs[i].name_off, recs[i].l_read_name ? recs[i].l_read_name - 1 : 0); };
    // what the reference swallows in mid-run (a partial result without a word) stops the run here, naming the read: every record that
    // reaches fromSAMRecord (L128) goes through its casts and, when it is not null, its CIGAR walk (LongreadRecord L102-190)
    std::vector<int32_t> bad_walk(h->cfg.n_threads, -1);
    {
        const int nt = std::max(1, std::min<int>(h->cfg.n_threads, (n + 4095) / 4096));
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++)
            th.emplace_back([&, t] {
                std::vector<int2> junc;
                for (int32_t i = (int32_t)((int64_t)n * t / nt); i < (int32_t)((int64_t)n * (t + 1) / nt); i++)
                    if ((flags[i] & kRecNotNull) && (recs[i].n_cigar == 0 || !lr::walk_junctions(bam, recs[i], junc))) {
                        bad_walk[t] = i;
                        break;
                    }
            });
        for (auto &x : th) x.join();
    }
    int32_t first_walk = -1;
    for (int32_t x : bad_walk)
        if (x >= 0 && (first_walk < 0 || x < first_walk)) first_walk = x;
    for (int32_t i = 0; i < n; i++) {
        if (flags[i] & kRecBadAux) {
            set_error("SNPMatrix: read " + name_of(i) + ": malformed attributes");
            return SMI_ERR_INVALID;
        }
        if (flags[i] & kRecBadType) {
            set_error("SNPMatrix: read " + name_of(i) + ": an attribute (CELLTAG, UMITAG, GENETAG, RNTAG, de or df) is not of the type SNPMatrix reads");
            return SMI_ERR_INVALID;
        }
        if (i == first_walk) {
            set_error("SNPMatrix: read " + name_of(i) + (recs[i].n_cigar == 0 ? ": no CIGAR" : ": the CIGAR walk runs past the alignment blocks"));
            return SMI_ERR_INVALID;
        }
    }
    const uint16_t umi_tag = lr::tag16(h->cfg.umi_tag);
    for (const SnpPair &p : pairs) {
        if (p.status & kPairNoQual) {
            set_error("SNPMatrix: read " + name_of(p.rec) + ": no base qualities (*) under a position of SNP line '" + h->lines[p.line].gene + "'");
            return SMI_ERR_INVALID;
        }
        if (p.status & kPairNoUmi) {
            set_error("SNPMatrix: read " + name_of(p.rec) + ": a hit of cell " + h->cells[p.cell] + " without the UMI attribute " + h->cfg.umi_tag);
            return SMI_ERR_INVALID;
        }
        Line &L = h->lines[p.line];
        const uint32_t st = p.status & kStatusMask;
        L.cnt[st]++;
        h->counts[SMI_SNP_PAIRS]++;
        h->counts[st == kHit ? SMI_SNP_HITS : st == kLowRn ? SMI_SNP_LOWRN : SMI_SNP_LOWQV]++;
        if (st != kHit || p.cell < 0) continue;  // Matrix.addMolecule L69: cells of the list only
        std::string_view umi;
        const uint8_t *q = bam + recs[p.rec].aux_off, *end = q + recs[p.rec].aux_len;
        while (q < end) {
            size_t k;
            if (lr::aux_size(q, end, &k)) break;
            if ((uint16_t)(q[0] | q[1] << 8) == umi_tag) umi = std::string_view((const char *)q + 3, k - 4);
            q += k;
        }
        auto it = h->umi_id.emplace(std::string(umi), (int32_t)h->umis.size());
        if (it.second) h->umis.push_back(it.first->first);
        h->hits.push_back(Hit{p.line, p.cell, it.first->second, p.rn, (uint64_t)h->hit_bq.size()});
        h->hit_bq.insert(h->hit_bq.end(), bq.begin() + p.byte_off, bq.begin() + p.byte_off + 2ull * p.npos);
    }
    return SMI_OK;
}

extern "C" int smi_snp_run(smi_snp *h, float *stage_ms) {
    if (!h) {
        set_error("smi_snp_run: null argument");
        return SMI_ERR_INVALID;
    }
    if (stage_ms) std::memset(stage_ms, 0, sizeof(h->ms));
    if (h->ran) {
        set_error("smi_snp_run: already run");
        return SMI_ERR_STATE;
    }
    h->ran = true;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    int64_t *c = h->counts;
    // molinfos order: the order the reference adds the molecules in -- line by line, records in file order
    std::stable_sort(h->hits.begin(), h->hits.end(), [](const Hit &x, const Hit &y) { return x.line < y.line; });
    const size_t nh = h->hits.size();
    c[SMI_SNP_KEPT] = (int64_t)nh;
    // rows: geneId \t chrom:pos|pos..bases (L171-172), interned per (line, bases), merged by their text, in byte order
    auto bases_of = [&](const Hit &x) {
        const size_t P = h->lines[x.line].arr.size();
        std::string b;
        for (size_t k = 0; k < P; k++)
            if (h->hit_bq[x.bq_off + k]) b += (char)h->hit_bq[x.bq_off + k];  // (0: complementBase's empty string)
        return b;
    };
    std::unordered_map<std::string, int32_t> row_of_key, row_of_label;
    std::vector<std::string> labels;
    std::vector<int32_t> hit_row(nh);
    for (size_t i = 0; i < nh; i++) {
        const Hit &x = h->hits[i];
        const Line &L = h->lines[x.line];
        std::string b = bases_of(x);
        std::string key = std::to_string(x.line) + ":" + b;
        auto kit = row_of_key.find(key);
        if (kit == row_of_key.end()) {
            std::string label = L.gene + "\t" + L.chrom + ":" + L.pos_text + ".." + b;
            auto lit = row_of_label.emplace(label, (int32_t)labels.size());
            if (lit.second) labels.push_back(std::move(label));
            kit = row_of_key.emplace(std::move(key), lit.first->second).first;
        }
        hit_row[i] = kit->second;
    }
    const size_t nrows = labels.size();
    std::vector<int32_t> ord(nrows), rank(nrows);
    for (size_t k = 0; k < nrows; k++) ord[k] = (int32_t)k;
    std::sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return labels[x] < labels[y]; });
    std::vector<std::string> rows(nrows), row_lab(nrows);
    for (size_t k = 0; k < nrows; k++) {
        rank[ord[k]] = (int32_t)k;
        rows[k] = labels[ord[k]];
        row_lab[k] = rows[k] + "\tna";  // writeIsoformMatrix with a null model (L190-193)
    }
    c[SMI_SNP_ROWS] = (int64_t)nrows;
    if (stage_ms) std::memcpy(stage_ms, h->ms, sizeof(h->ms));
    if (nrows == 0) return SMI_OK;  // L209-210: nothing detected, no file
    if (nh > (size_t)INT32_MAX) {
        set_error("SNPMatrix: " + std::to_string(nh) + " hits; at most 2^31 - 1 are counted in one sort");
        return SMI_ERR_INVALID;
    }
    // distinct UMIs per (row, cell): sort (row, cell, UMI id), drop the repeats
    std::vector<uint64_t> codes(nh);
    std::vector<uint32_t> umi(nh);
    for (size_t i = 0; i < nh; i++) {
        codes[i] = (uint64_t)(uint32_t)rank[hit_row[i]] << 32 | (uint32_t)h->hits[i].cell;
        umi[i] = (uint32_t)h->hits[i].umi;
    }
    {
        DevBuf<uint64_t> d_c0{kWho}, d_c1{kWho}, d_sel{kWho};
        DevBuf<uint32_t> d_u0{kWho}, d_u1{kWho};
        DevBuf<uint8_t> d_first{kWho};
        Scratch tmp{kWho};
        DevBuf<int64_t> d_nsel{kWho};
        int rc;
        if ((rc = d_c0.put(codes, s)) || (rc = d_u0.put(umi, s)) || (rc = d_c1.alloc(nh)) || (rc = d_u1.alloc(nh)) || (rc = d_sel.alloc(nh)) ||
            (rc = d_first.alloc(nh)) || (rc = d_nsel.alloc(1)))
            return rc;
        int umi_bits = 1, end_bit = 32;
        while (umi_bits < 32 && ((uint64_t)1 << umi_bits) < h->umis.size()) umi_bits++;
        while (end_bit < 64 && ((uint64_t)1 << (end_bit - 32)) < (uint64_t)nrows) end_bit++;
        const auto by_umi = [&](void *p, size_t &t) { return hipcub::DeviceRadixSort::SortPairs(p, t, d_u0.p, d_u1.p, d_c0.p, d_c1.p, (int)nh, 0, umi_bits, s); };
        const auto by_code = [&](void *p, size_t &t) { return hipcub::DeviceRadixSort::SortPairs(p, t, d_c1.p, d_c0.p, d_u1.p, d_u0.p, (int)nh, 0, end_bit, s); };
        const auto select = [&](void *p, size_t &t) { return hipcub::DeviceSelect::Flagged(p, t, d_c0.p, d_first.p, d_sel.p, d_nsel.p, (int)nh, s); };
        if ((rc = reserve(tmp, by_umi, by_code, select))) return rc;
        Events ev;
        if ((rc = ev.begin(s))) return rc;
        if ((rc = run_reserved(tmp, by_umi)) || (rc = run_reserved(tmp, by_code))) return rc;
        hipLaunchKernelGGL(k_snp_first, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, s, d_c0.p, d_u0.p, (int64_t)nh, d_first.p);
        SMI_HIP(hipGetLastError());
        if ((rc = run_reserved(tmp, select))) return rc;
        if ((rc = ev.end(s, &h->ms[1]))) return rc;
        int64_t nsel = 0;
        SMI_HIP(hipMemcpy(&nsel, d_nsel.p, sizeof(nsel), hipMemcpyDeviceToHost));
        codes.resize(nsel);
        SMI_HIP(hipMemcpy(codes.data(), d_sel.p, nsel * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    std::string head;
    for (auto &cell : h->cells) head += "\t" + cell;
    head += "\n";
    std::vector<int64_t> tot;
    std::string &mat = h->out[SMI_SNP_OUT_MATRIX];
    mat = "geneId\ttranscriptId\tnbExons" + head;
    if (int rc = mtx::matrix(s, "SNPMatrix", (int32_t)h->cells.size(), h->cfg.budget_bytes, codes, row_lab, mat, tot, &h->ms[1], &h->ms[2],
                             &c[SMI_SNP_RENDER_BLOCKS]))
        return rc;
    SMI_HIP(hipStreamSynchronize(s));
    std::string &met = h->out[SMI_SNP_OUT_METRICS];
    met = "geneId\ttranscriptId\tnbExons\tnbUmis\n";
    for (size_t r = 0; r < nrows; r++) {
        met += row_lab[r] + "\t" + std::to_string(tot[r]) + "\n";
        c[SMI_SNP_TOTAL_COUNT] += tot[r];
    }
    // Matrix.java L209-214: nbReads = rn if rn > 1, else the molecule's one read; nbSupportingReads 0; pctId an unset Float ("null")
    std::string &mol = h->out[SMI_SNP_OUT_MOLINFOS];
    mol = "cellBC\tUMI\tnbReads\tnbSupportingReads\tmappingPctId\tsnpPhredScore\tgeneId\ttranscriptId\n";
    for (size_t i = 0; i < nh; i++) {
        const Hit &x = h->hits[i];
        const size_t P = h->lines[x.line].arr.size();
        mol += h->cells[x.cell] + "\t" + h->umis[x.umi] + "\t" + std::to_string(x.rn > 1 ? x.rn : 1) + "\t0\tnull\t";
        for (size_t k = 0; k < P; k++) {
            if (k) mol += ',';
            mol += std::to_string((int)h->hit_bq[x.bq_off + P + k]);
        }
        mol += "\t" + labels[hit_row[i]] + "\n";
    }
    if (stage_ms) std::memcpy(stage_ms, h->ms, sizeof(h->ms));
    return SMI_OK;
}

extern "C" int smi_snp_output(const smi_snp *h, int32_t which, uint8_t *out, size_t cap, size_t *n_out) {
    if (!h || !n_out || which < 0 || which >= SMI_SNP_OUTPUTS) {
        set_error("smi_snp_output: bad argument");
        return SMI_ERR_INVALID;
    }
    return handle::get_text(h->out[which], out, cap, n_out);
}

extern "C" int smi_snp_counts(const smi_snp *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_snp_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof(h->counts));
    return SMI_OK;
}

extern "C" int smi_snp_line_counts(const smi_snp *h, int64_t *counts, size_t cap_lines, size_t *n_lines) {
    if (!h || !n_lines) {
        set_error("smi_snp_line_counts: null argument");
        return SMI_ERR_INVALID;
    }
    *n_lines = h->text_line.size();
    if (!counts) return SMI_OK;
    if (cap_lines < h->text_line.size()) return 1;
    for (size_t i = 0; i < h->text_line.size(); i++)
        for (int k = 0; k < 3; k++) counts[3 * i + k] = h->text_line[i] < 0 ? -1 : h->lines[h->text_line[i]].cnt[k];
    return SMI_OK;
}
