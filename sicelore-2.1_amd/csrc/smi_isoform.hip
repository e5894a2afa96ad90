// smi_isoform.hip -- `IsoformMatrix` (org/ipmc/sicelore/programs/IsoformMatrix.java:L93-160), STRICT method: K-ISO assigns every
// molecule its transcript on the device, K-MTX counts and renders the three dense matrices; the refFlat model, the cell list, the record
// parser, the read and molecule grouping and the metrics files are host work.  The rules are DESIGN.md section 8d's; tests/isoformmodel.py
// implements the same ones.
//
// Host, in the reference's order:
//   model     UCSCRefFlatParser(File) L44-77 over TranscriptRecord.fromRefFlat: exons (start + 1, end), junctions (exon[i-1].end,
//             exon[i].start); a line whose exon bases sum to 0 is dropped; transcripts grouped by gene (column 0) in file order.  A line of
//             fewer than 11 fields or with a bad integer ends the reference's parse silently: here it fails the call naming the line.
//             Keys `txId|geneId` are interned (ids in byte order of the key), so that duplicate lines of one transcript count as one
//             candidate; select(gene, tx) (L114-125) = the last line of the key.
//   cells     CellList: one barcode per line, every "-1" removed, duplicates collapse; columns in byte order.
//   records   LongreadParser.parseSAMRecord over LongreadRecord.fromSAMRecord(r, load_sequence = false) with gene and UMI mandatory:
//             null / unmapped -> chimeric -> no gene (null, "" or "undef") -> no UMI -> mapq 0 and secondary / supplementary unless
//             MAPQV0.  The junction list is the literal walk of L120-150 (see walk_junctions).  A cast the reference would fail, a mapped
//             record without CIGAR or alignment block, or a walk past the last block fails the call with the read's name.
//   reads     by name in order of the first kept record; barcode, UMI and rn of the last record; genes = union of GENETAG split on ','.
//   molecules `barcode:umi` in order of their first read; rn of the first read; pctId = 1f - de of the first record of the last read.
// K-ISO: one wavefront per molecule (setIsoformStrictNew, MoleculeDataset.java L161-236): lanes over (record, transcript) pairs, the
//   match test of map() per pair, candidate counts per candidate transcript in LDS (in an HBM slice when the molecule has more than
//   lds_tx transcripts), counts summed per key; best / tie (smallest key) / monoexon / nomatch (most lines, then first gene); then the
//   molecule's junction set as ids of the table of unique model junctions (a second launch writes them at the scanned offsets).
// K-MTX: 64-bit (row << 32 | cell) codes per counted molecule; hipcub radix sort + run-length encoding give the UMI counts (a molecule is
//   one UMI of its cell); the dense rows are rendered in row blocks under a device-memory budget, one wavefront per row: a length pass, a
//   scan, the write (smi_mtx.h, shared with SNPMatrix).
#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstring>
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

constexpr const char *kWho = "IsoformMatrix";  // the program named when a device allocation fails

constexpr int kIsoWaves = 4;     // waves per block of K-ISO
constexpr int kLdsTx = 2048;     // candidate counts of one wave held in LDS

enum IsoStatus : int32_t { kNone = 0, kMono = 1, kOne = 2, kAmbiguous = 3, kNomatch = 4 };

struct IsoArgs {
    const int32_t *mol_rec_off;   // n_mol + 1: records of molecule m (reads in order, records in order)
    const int32_t *rec_j_off;     // n_rec + 1: junctions of record r in rj
    const int2 *rj;
    const int32_t *mol_gene_off;  // n_mol + 1: the molecule's model genes, ascending
    const int32_t *mol_gene;
    const int32_t *gene_tx_off;   // n_gene + 1: transcripts (refFlat lines) of gene g in file order
    const int32_t *gene_tx;
    const int32_t *tx_j_off;      // n_tx + 1: junctions of line t in tj
    const int2 *tj;
    const int32_t *tx_key;        // key id of line t (`txId|geneId` in byte order)
    const int32_t *tx_rep;        // position in its gene's list of the first line of line t's key (duplicate lines count there)
    const int32_t *gene_u_off;    // n_gene + 1: unique junction ids of gene g, ascending
    const int32_t *gene_u;
    const int2 *ujunc;            // the unique model junctions
    int32_t n_mol, delta, lds_tx;
    const int64_t *spill_off;     // per molecule: offset of its counts in spill, or -1 (they fit in LDS)
    int32_t *spill;
    int32_t *out_key, *out_gene, *out_status, *out_support, *out_njunc;
    const int64_t *junc_off;      // WRITE: molecule m's junction ids go to junc_out[junc_off[m] ..)
    int32_t *junc_out;
};

// the j-th candidate transcript of a molecule (genes in order, their lines in file order); *base: the index of its gene's first line
__device__ __forceinline__ int tx_of(const IsoArgs &a, int g0, int g1, int j, int *base = nullptr) {
    int b = 0;
    for (int g = g0; g < g1; g++) {
        const int gene = a.mol_gene[g];
        const int n = a.gene_tx_off[gene + 1] - a.gene_tx_off[gene];
        if (j < n) {
            if (base) *base = b;
            return a.gene_tx[a.gene_tx_off[gene] + j];
        }
        j -= n;
        b += n;
    }
    return -1;
}

__device__ __forceinline__ long long wave_max64(long long v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (long long)__shfl_xor(v, o));
    return v;
}

// COUNT: the assignment and the size of the junction set; WRITE: the junction set at junc_off
template <bool WRITE>
__global__ __launch_bounds__(64 * kIsoWaves) void k_iso(IsoArgs a) {
    __shared__ int32_t lds_cnt[kIsoWaves][kLdsTx];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m = blockIdx.x * kIsoWaves + wv;
    if (m >= a.n_mol) return;
    const int g0 = a.mol_gene_off[m], g1 = a.mol_gene_off[m + 1];
    const int r0 = a.mol_rec_off[m], r1 = a.mol_rec_off[m + 1];
    const int j0 = a.rec_j_off[r0], j1 = a.rec_j_off[r1];  // every junction of every record of the molecule
    int nT = 0;
    for (int g = g0; g < g1; g++) nT += a.gene_tx_off[a.mol_gene[g] + 1] - a.gene_tx_off[a.mol_gene[g]];
    const int d = a.delta;
    const bool mono = nT == 1 && a.tx_j_off[tx_of(a, g0, g1, 0) + 1] == a.tx_j_off[tx_of(a, g0, g1, 0)];
    if (!WRITE) {
        int32_t key = -1, gene = -1, status = kNone, support = 0;
        if (mono) {
            const int t = tx_of(a, g0, g1, 0);
            key = a.tx_key[t];
            status = kMono;
            support = 1;
        } else if (nT > 0) {
            int32_t *cnt = a.spill_off[m] >= 0 ? a.spill + a.spill_off[m] : lds_cnt[wv];
            for (int j = lane; j < nT; j += 64) cnt[j] = 0;
            __threadfence_block();
            wave_sync();
            const int nR = r1 - r0;
            for (long long p = lane; p < (long long)nR * nT; p += 64) {  // map(readJ, refJ, DELTA) per (record, transcript)
                const int r = r0 + (int)(p / nT), j = (int)(p % nT);
                int base = 0;
                const int t = tx_of(a, g0, g1, j, &base);
                const int nr = a.rec_j_off[r + 1] - a.rec_j_off[r];
                const int nt = a.tx_j_off[t + 1] - a.tx_j_off[t];
                if (nt == 0 || nt != nr) continue;
                const int2 *rl = a.rj + a.rec_j_off[r];
                const int2 *tl = a.tj + a.tx_j_off[t];
                bool ok = true;
                for (int k = 0; k < nt && ok; k++) ok = is_in(tl[k], rl, nr, d);
                if (ok) atomicAdd(&cnt[base + a.tx_rep[t]], 1);  // counted per key: at the key's first line
            }
            __threadfence_block();
            wave_sync();
            // one entry per key (at its first line); best = the highest count, then the smallest key
            long long best = -1;
            for (int j = lane; j < nT; j += 64)
                if (cnt[j] > 0) best = max(best, (long long)cnt[j] << 32 | (long long)(0x7fffffff - a.tx_key[tx_of(a, g0, g1, j)]));
            best = wave_max64(best);
            if (best > 0) {
                const int bk = 0x7fffffff - (int)(best & 0xffffffff), btot = (int)(best >> 32);
                int tied = 0;
                for (int j = lane; j < nT; j += 64) tied += cnt[j] == btot;
                for (int o = 32; o > 0; o >>= 1) tied += __shfl_xor(tied, o);
                key = bk;
                support = btot;
                status = tied > 1 ? kAmbiguous : kOne;
            } else {  // getGeneIdForMostComplexTranscript: the gene of the most lines, the first gene on a tie
                status = kNomatch;
                int bn = -1;
                for (int g = g0; g < g1; g++) {
                    const int n = a.gene_tx_off[a.mol_gene[g] + 1] - a.gene_tx_off[a.mol_gene[g]];
                    if (n > bn) {
                        bn = n;
                        gene = a.mol_gene[g];
                    }
                }
            }
        }
        if (lane == 0) {
            a.out_key[m] = key;
            a.out_gene[m] = gene;
            a.out_status[m] = status;
            a.out_support[m] = support;
        }
    }
    // the junction set (map() L291-296 for every (record, transcript) pair): every unique junction of the candidate genes that is isIn
    // some junction of some record; none for a monoexon molecule (the match loop does not run)
    int n_out = 0;
    if (!mono) {
        for (int g = g0; g < g1; g++) {
            const int gene = a.mol_gene[g];
            const int u0 = a.gene_u_off[gene], u1 = a.gene_u_off[gene + 1];
            for (int base = u0; base < u1; base += 64) {
                const int ui = base + lane;
                bool keep = false;
                int u = -1;
                if (ui < u1) {
                    u = a.gene_u[ui];
                    keep = is_in(a.ujunc[u], a.rj + j0, j1 - j0, d);
                    for (int h = g0; h < g && keep; h++) {  // already taken from an earlier gene of the molecule
                        const int og = a.mol_gene[h];
                        int lo = a.gene_u_off[og], hi = a.gene_u_off[og + 1];
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (a.gene_u[mid] < u) lo = mid + 1;
                            else hi = mid;
                        }
                        if (lo < a.gene_u_off[og + 1] && a.gene_u[lo] == u) keep = false;
                    }
                }
                const unsigned long long bal = __ballot(keep);
                if (WRITE && keep) {
                    const int before = __popcll(bal & ((1ull << lane) - 1ull));
                    a.junc_out[a.junc_off[m] + n_out + before] = u;
                }
                n_out += __popcll(bal);
            }
        }
    }
    if (!WRITE && lane == 0) a.out_njunc[m] = n_out;
}


// ---- host parsing -----------------------------------------------------------------------------------------------------------------------
using lr::drop_minus1;
using lr::java_float;
using lr::jsplit;

struct Model {
    std::vector<std::string> genes;             // model genes in order of their first line
    std::unordered_map<std::string, int32_t> gene_id;
    std::vector<int32_t> tx_gene, tx_key, tx_rep, tx_nexon, tx_j_off{0};
    std::vector<int2> tj;
    std::vector<int32_t> gene_tx_off, gene_tx;  // CSR
    std::vector<std::string> key_tx, key_gene;  // per key id (byte order of txId|geneId)
    std::vector<int32_t> key_nexon;             // select(gene, tx): the last line of the key
    std::vector<int2> ujunc;                    // unique (start, end), ascending
    std::vector<int32_t> gene_u_off, gene_u;
    int64_t n_lines = 0;
};

int parse_model(const char *text, size_t n, Model &M) {
    std::vector<std::string> line_tx;
    std::unordered_map<std::string, int32_t> key_of;
    std::vector<std::string> key_str;
    std::vector<int32_t> line_key;
    std::vector<int32_t> line_gene;
    size_t b = 0;
    int64_t lineno = 0;
    std::vector<std::vector<int32_t>> by_gene;
    handle::RefFlatLine L;
    std::string err;
    while (b < n) {
        size_t e = b;
        while (e < n && text[e] != '\n') e++;
        const int kind = handle::refflat_line("IsoformMatrix", std::string_view(text + b, e - b), ++lineno, false, L, err);
        b = e + 1;
        if (kind == handle::kLineBad) {
            set_error(err);
            return SMI_ERR_INVALID;
        }
        if (kind == handle::kLineDropped) continue;
        const std::vector<int32_t> &xs = L.xs, &xe = L.xe;
        M.n_lines++;
        const std::string gname(L.gene);
        auto git = M.gene_id.emplace(gname, (int32_t)M.genes.size());
        if (git.second) {
            M.genes.push_back(gname);
            by_gene.emplace_back();
        }
        const int32_t t = (int32_t)M.tx_gene.size();
        M.tx_gene.push_back(git.first->second);
        by_gene[git.first->second].push_back(t);
        M.tx_nexon.push_back((int32_t)xs.size());
        for (size_t i = 1; i < xs.size(); i++) M.tj.push_back(make_int2(xe[i - 1], xs[i] + 1));
        M.tx_j_off.push_back((int32_t)M.tj.size());
        std::string key = std::string(L.tx) + "|" + gname;
        auto kit = key_of.emplace(key, (int32_t)key_str.size());
        if (kit.second) {
            key_str.push_back(key);
            line_tx.push_back(std::string(L.tx));
            line_gene.push_back(git.first->second);
        }
        line_key.push_back(kit.first->second);
    }
    // key ids in byte order of the key
    std::vector<int32_t> ord(key_str.size()), rank(key_str.size());
    for (size_t i = 0; i < ord.size(); i++) ord[i] = (int32_t)i;
    std::sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return key_str[x] < key_str[y]; });
    M.key_tx.resize(ord.size());
    M.key_gene.resize(ord.size());
    M.key_nexon.assign(ord.size(), 0);
    for (size_t i = 0; i < ord.size(); i++) {
        rank[ord[i]] = (int32_t)i;
        M.key_tx[i] = line_tx[ord[i]];
        M.key_gene[i] = M.genes[line_gene[ord[i]]];
    }
    M.tx_key.resize(line_key.size());
    for (size_t t = 0; t < line_key.size(); t++) {
        M.tx_key[t] = rank[line_key[t]];
        M.key_nexon[M.tx_key[t]] = M.tx_nexon[t];  // the last line wins
    }
    M.gene_tx_off.assign(1, 0);
    M.tx_rep.assign(M.tx_key.size(), 0);
    for (auto &l : by_gene) {
        M.gene_tx.insert(M.gene_tx.end(), l.begin(), l.end());
        M.gene_tx_off.push_back((int32_t)M.gene_tx.size());
        for (size_t i = 0; i < l.size(); i++) {  // a key's lines are all in one gene (the key holds the gene)
            size_t f = 0;
            while (M.tx_key[l[f]] != M.tx_key[l[i]]) f++;
            M.tx_rep[l[i]] = (int32_t)f;
        }
    }
    // unique junctions and per gene the ascending ids of its junctions
    M.ujunc = M.tj;
    auto lt = [](int2 x, int2 y) { return x.x != y.x ? x.x < y.x : x.y < y.y; };
    std::sort(M.ujunc.begin(), M.ujunc.end(), lt);
    M.ujunc.erase(std::unique(M.ujunc.begin(), M.ujunc.end(), [](int2 x, int2 y) { return x.x == y.x && x.y == y.y; }), M.ujunc.end());
    M.gene_u_off.assign(1, 0);
    for (auto &l : by_gene) {
        std::vector<int32_t> u;
        for (int32_t t : l)
            for (int32_t k = M.tx_j_off[t]; k < M.tx_j_off[t + 1]; k++)
                u.push_back((int32_t)(std::lower_bound(M.ujunc.begin(), M.ujunc.end(), M.tj[k], lt) - M.ujunc.begin()));
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
        M.gene_u.insert(M.gene_u.end(), u.begin(), u.end());
        M.gene_u_off.push_back((int32_t)M.gene_u.size());
    }
    return SMI_OK;
}

}  // namespace
}  // namespace smi

using namespace smi;

struct smi_isoform {
    smi_ctx *ctx = nullptr;
    smi_isoform_config cfg = {};
    lr::TagSet tags;
    Model M;
    std::vector<std::string> cells;  // byte order
    std::unordered_map<std::string, int32_t> cell_id;
    // kept records in file order
    std::string text;
    std::vector<uint64_t> name_off, bc_off, umi_off, gene_off;
    std::vector<uint32_t> name_len, bc_len, umi_len, gene_len;
    std::vector<float> de;
    std::vector<int32_t> rn, rj_off{0};
    std::vector<int2> rj;
    int64_t counts[SMI_ISOFORM_COUNTS] = {};
    std::string out[SMI_ISOFORM_OUTPUTS];
    bool ran = false;
    // ISOBAM: molecules by `barcode:umi`, entry 0 = undef / undef, entry m + 1 = molecule m's IG / IT in iso_text
    std::unordered_map<std::string, int32_t> mol_by_key;
    std::vector<uint8_t> iso_text;
    std::vector<uint64_t> ig_start, it_start;
    std::vector<uint32_t> ig_len, it_len;
    uint8_t *d_iso_text = nullptr;
    uint64_t *d_ig_start = nullptr, *d_it_start = nullptr;
    uint32_t *d_ig_len = nullptr, *d_it_len = nullptr;
    std::vector<uint8_t> isobam;  // the last segment's records
    const uint8_t *last_bam = nullptr;
    const smi_bam_record *last_recs = nullptr;
    int32_t last_n = -1;
    float isobam_ms = 0.f;
    ~smi_isoform() {
        for (void *p : {(void *)d_iso_text, (void *)d_ig_start, (void *)d_it_start, (void *)d_ig_len, (void *)d_it_len})
            if (p) (void)hipFree(p);
    }
};

extern "C" int smi_isoform_default_config(smi_isoform_config *cfg) {
    if (!cfg) {
        set_error("smi_isoform_default_config: null argument");
        return SMI_ERR_INVALID;
    }
    *cfg = {};
    std::memcpy(cfg->cell_tag, "BC", 3);
    std::memcpy(cfg->umi_tag, "U8", 3);
    std::memcpy(cfg->gene_tag, "GE", 3);
    std::memcpy(cfg->rn_tag, "RN", 3);
    cfg->max_clip = 150;
    cfg->mapqv0 = 0;
    cfg->delta = 2;
    cfg->to_bulk = 0;
    cfg->n_threads = 20;
    cfg->lds_tx = kLdsTx;
    cfg->budget_bytes = 0;
    return SMI_OK;
}

extern "C" int smi_isoform_create(smi_ctx *ctx, const smi_isoform_config *cfg, const char *refflat, size_t n_refflat, const char *csv, size_t n_csv,
                                  smi_isoform **out) {
    if (!ctx || !cfg || !out || (n_refflat && !refflat) || (n_csv && !csv)) {
        set_error("smi_isoform_create: null argument");
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
    if (cfg->delta < 0) {
        set_error("DELTA must be 0 or more");
        return SMI_ERR_INVALID;
    }
    if (cfg->lds_tx < 1 || cfg->lds_tx > kLdsTx) {
        set_error("smi_isoform_config.lds_tx must be 1 .. " + std::to_string(kLdsTx));
        return SMI_ERR_INVALID;
    }
    smi_isoform *h = new smi_isoform();
    h->ctx = ctx;
    h->cfg = *cfg;
    h->cfg.n_threads = std::max(1, std::min(cfg->n_threads, 256));
    h->tags.set(lr::kCell, cfg->cell_tag).set(lr::kUmi, cfg->umi_tag).set(lr::kGene, cfg->gene_tag).set(lr::kRn, cfg->rn_tag);
    if (int rc = parse_model(refflat, n_refflat, h->M)) {
        delete h;
        return rc;
    }
    std::vector<std::string> cells = handle::cell_list(csv, n_csv);
    std::sort(cells.begin(), cells.end());
    cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
    h->cells = std::move(cells);
    for (size_t i = 0; i < h->cells.size(); i++) h->cell_id.emplace(h->cells[i], (int32_t)i);
    h->counts[SMI_ISO_GENES] = (int64_t)h->M.genes.size();
    h->counts[SMI_ISO_TRANSCRIPTS] = h->M.n_lines;
    h->counts[SMI_ISO_CELLS] = (int64_t)h->cells.size();
    *out = h;
    return SMI_OK;
}

extern "C" int smi_isoform_free(smi_isoform *h) {
    delete h;
    return SMI_OK;
}

extern "C" int smi_isoform_add_segment(smi_isoform *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n) {
    if (!h || n < 0 || (n && (!bam || !recs))) {
        set_error("smi_isoform_add_segment: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->ran) {
        set_error("smi_isoform_add_segment: the matrices were already built (smi_isoform_run)");
        return SMI_ERR_STATE;
    }
    const lr::Segment seg = lr::read_segment("smi_isoform_add_segment", bam, n_bam, recs, n, h->cfg.n_threads,
                                             [&](const uint8_t *b, const smi_bam_record &r, lr::Record &out, std::string &err) {
                                                 lr::read_isoform(b, r, h->tags, h->cfg.max_clip, h->cfg.mapqv0, out, err);
                                             });
    if (!seg.refused.empty()) {
        set_error(seg.refused);
        return SMI_ERR_INVALID;
    }
    if (seg.first_error >= 0) {
        set_error("IsoformMatrix: read " + std::string(lr::read_name(bam, recs[seg.first_error])) + ": " + seg.error);
        return SMI_ERR_INVALID;
    }
    int64_t *c = h->counts;
    auto put = [&](std::string_view s, std::vector<uint64_t> &off, std::vector<uint32_t> &len) {
        off.push_back(h->text.size());
        len.push_back((uint32_t)s.size());
        h->text.append(s);
    };
    for (int32_t i = 0; i < n; i++) {
        const lr::Record &p = seg.recs[i];
        c[SMI_ISO_RECORDS]++;
        if (p.what != lr::kKept) {
            c[SMI_ISO_UNVALID]++;
            c[p.what == lr::kNull ? SMI_ISO_NULL : p.what == lr::kChimeric ? SMI_ISO_CHIMERIA : p.what == lr::kNoGene ? SMI_ISO_NO_GENE
              : p.what == lr::kNoUmi ? SMI_ISO_NO_UMI : SMI_ISO_MAPQV0]++;
            continue;
        }
        c[SMI_ISO_VALID]++;
        put(lr::read_name(bam, recs[i]), h->name_off, h->name_len);
        put(drop_minus1(p.bc), h->bc_off, h->bc_len);
        put(p.umi, h->umi_off, h->umi_len);
        put(p.gene, h->gene_off, h->gene_len);
        h->de.push_back(p.de);
        h->rn.push_back(p.rn);
        h->rj.insert(h->rj.end(), p.junc.begin(), p.junc.end());
        h->rj_off.push_back((int32_t)h->rj.size());
    }
    return SMI_OK;
}


extern "C" int smi_isoform_run(smi_isoform *h, float *stage_ms) {
    if (!h) {
        set_error("smi_isoform_run: null argument");
        return SMI_ERR_INVALID;
    }
    float ms[SMI_ISOFORM_STAGES] = {};
    if (stage_ms) std::memset(stage_ms, 0, sizeof(ms));
    if (h->ran) {
        set_error("smi_isoform_run: already run");
        return SMI_ERR_STATE;
    }
    h->ran = true;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    const Model &M = h->M;
    const char *T = h->text.data();
    auto sv = [&](const std::vector<uint64_t> &off, const std::vector<uint32_t> &len, size_t i) { return std::string_view(T + off[i], len[i]); };
    const size_t nk = h->de.size();
    int64_t *c = h->counts;
    // reads by name in order of their first kept record
    std::unordered_map<std::string_view, int32_t> by_name;
    by_name.reserve(nk * 2 + 1);
    std::vector<int32_t> read_first, read_last, rec_read(nk);
    std::vector<int32_t> read_n;
    for (size_t i = 0; i < nk; i++) {
        auto it = by_name.emplace(sv(h->name_off, h->name_len, i), (int32_t)read_first.size());
        if (it.second) {
            read_first.push_back((int32_t)i);
            read_last.push_back((int32_t)i);
            read_n.push_back(1);
        } else {
            read_last[it.first->second] = (int32_t)i;
            read_n[it.first->second]++;
        }
        rec_read[i] = it.first->second;
    }
    const size_t n_reads = read_first.size();
    c[SMI_ISO_READS] = (int64_t)n_reads;
    for (int32_t x : read_n) c[SMI_ISO_READS_MULTI] += x > 1;
    std::vector<int64_t> rstart(n_reads + 1, 0);
    for (size_t r = 0; r < n_reads; r++) rstart[r + 1] = rstart[r] + read_n[r];
    std::vector<int32_t> rrecs(nk), rfill(n_reads, 0);
    for (size_t i = 0; i < nk; i++) rrecs[rstart[rec_read[i]] + rfill[rec_read[i]]++] = (int32_t)i;
    // molecules keyed barcode:umi of the read's last record, in order of their first read
    std::unordered_map<std::string, int32_t> by_key;
    by_key.reserve(n_reads + 1);
    std::vector<int32_t> mol_of(n_reads), mol_n, mol_first_read, mol_last_read;
    for (size_t r = 0; r < n_reads; r++) {
        std::string key(sv(h->bc_off, h->bc_len, read_last[r]));
        key += ':';
        key.append(sv(h->umi_off, h->umi_len, read_last[r]));
        auto it = by_key.emplace(std::move(key), (int32_t)mol_n.size());
        if (it.second) {
            mol_n.push_back(0);
            mol_first_read.push_back((int32_t)r);
            mol_last_read.push_back((int32_t)r);
        }
        mol_of[r] = it.first->second;
        mol_n[it.first->second]++;
        mol_last_read[it.first->second] = (int32_t)r;
    }
    const size_t n_mol = mol_n.size();
    c[SMI_ISO_MOLECULES] = (int64_t)n_mol;
    std::vector<int64_t> mstart(n_mol + 1, 0);
    for (size_t m = 0; m < n_mol; m++) mstart[m + 1] = mstart[m] + mol_n[m];
    std::vector<int32_t> mreads(n_reads), mfill(n_mol, 0);
    for (size_t r = 0; r < n_reads; r++) mreads[mstart[mol_of[r]] + mfill[mol_of[r]]++] = (int32_t)r;
    c[SMI_ISO_MOLECULE_READS] = (int64_t)n_reads;
    // per molecule: records (CSR), its distinct genes (multiIG), its model genes (ascending)
    std::vector<int32_t> mol_rec_off{0}, mrec_j_off{0};
    std::vector<int2> mrj;
    std::vector<int32_t> mol_gene_off{0}, mol_gene;
    std::vector<std::string_view> gl;
    for (size_t m = 0; m < n_mol; m++) {
        gl.clear();
        for (int64_t k = mstart[m]; k < mstart[m + 1]; k++) {
            const int32_t r = mreads[k];
            for (int64_t q = rstart[r]; q < rstart[r + 1]; q++) {
                const int32_t i = rrecs[q];
                for (auto g : jsplit(sv(h->gene_off, h->gene_len, i), ',')) gl.push_back(g);
                mrj.insert(mrj.end(), h->rj.begin() + h->rj_off[i], h->rj.begin() + h->rj_off[i + 1]);
                mrec_j_off.push_back((int32_t)mrj.size());
            }
        }
        mol_rec_off.push_back((int32_t)mrec_j_off.size() - 1);
        std::sort(gl.begin(), gl.end());
        gl.erase(std::unique(gl.begin(), gl.end()), gl.end());
        c[SMI_ISO_MULTI_IG] += gl.size() > 1;
        const size_t before = mol_gene.size();
        for (auto g : gl) {
            auto it = M.gene_id.find(std::string(g));
            if (it != M.gene_id.end()) mol_gene.push_back(it->second);
        }
        std::sort(mol_gene.begin() + before, mol_gene.end());
        mol_gene_off.push_back((int32_t)mol_gene.size());
    }
    // spill slices for molecules of more candidate transcripts than the LDS holds
    std::vector<int64_t> spill_off(n_mol, -1);
    int64_t spill_n = 0;
    for (size_t m = 0; m < n_mol; m++) {
        int64_t nT = 0;
        for (int32_t g = mol_gene_off[m]; g < mol_gene_off[m + 1]; g++) nT += M.gene_tx_off[mol_gene[g] + 1] - M.gene_tx_off[mol_gene[g]];
        if (nT > h->cfg.lds_tx) {
            spill_off[m] = spill_n;
            spill_n += nT;
            c[SMI_ISO_SPILL]++;
        }
    }
    // K-ISO
    std::vector<int32_t> m_key(n_mol), m_gene(n_mol), m_status(n_mol), m_support(n_mol), m_nj(n_mol);
    std::vector<int32_t> jset;
    std::vector<int64_t> joff(n_mol + 1, 0);
    if (n_mol) {
        DevBuf<int32_t> d_mro{kWho}, d_rjo{kWho}, d_mgo{kWho}, d_mg{kWho}, d_gto{kWho}, d_gt{kWho}, d_tjo{kWho}, d_tk{kWho}, d_tr{kWho}, d_guo{kWho}, d_gu{kWho}, d_spill{kWho}, d_key{kWho}, d_gene{kWho}, d_st{kWho}, d_sup{kWho}, d_nj{kWho}, d_jout{kWho};
        DevBuf<int2> d_rj{kWho}, d_tj{kWho}, d_uj{kWho};
        DevBuf<int64_t> d_so{kWho}, d_jo{kWho};
        int rc = 0;
        if ((rc = d_mro.put(mol_rec_off, s)) || (rc = d_rjo.put(mrec_j_off, s)) || (rc = d_rj.put(mrj, s)) || (rc = d_mgo.put(mol_gene_off, s)) ||
            (rc = d_mg.put(mol_gene, s)) || (rc = d_gto.put(M.gene_tx_off, s)) || (rc = d_gt.put(M.gene_tx, s)) || (rc = d_tjo.put(M.tx_j_off, s)) ||
            (rc = d_tj.put(M.tj, s)) || (rc = d_tk.put(M.tx_key, s)) || (rc = d_tr.put(M.tx_rep, s)) || (rc = d_guo.put(M.gene_u_off, s)) || (rc = d_gu.put(M.gene_u, s)) ||
            (rc = d_uj.put(M.ujunc, s)) || (rc = d_so.put(spill_off, s)) || (rc = d_spill.alloc(spill_n)) || (rc = d_key.alloc(n_mol)) ||
            (rc = d_gene.alloc(n_mol)) || (rc = d_st.alloc(n_mol)) || (rc = d_sup.alloc(n_mol)) || (rc = d_nj.alloc(n_mol)))
            return rc;
        IsoArgs a = {d_mro.p, d_rjo.p, d_rj.p, d_mgo.p, d_mg.p, d_gto.p, d_gt.p, d_tjo.p, d_tj.p, d_tk.p, d_tr.p, d_guo.p, d_gu.p, d_uj.p,
                     (int32_t)n_mol, h->cfg.delta, h->cfg.lds_tx, d_so.p, d_spill.p, d_key.p, d_gene.p, d_st.p, d_sup.p, d_nj.p, nullptr, nullptr};
        const unsigned grid = (unsigned)((n_mol + kIsoWaves - 1) / kIsoWaves);
        Events ev;
        if ((rc = ev.begin(s))) return rc;
        hipLaunchKernelGGL(k_iso<false>, dim3(grid), dim3(64 * kIsoWaves), 0, s, a);
        SMI_HIP(hipGetLastError());
        if ((rc = ev.end(s, &ms[0]))) return rc;
        SMI_HIP(hipMemcpy(m_key.data(), d_key.p, n_mol * 4, hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(m_gene.data(), d_gene.p, n_mol * 4, hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(m_status.data(), d_st.p, n_mol * 4, hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(m_support.data(), d_sup.p, n_mol * 4, hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(m_nj.data(), d_nj.p, n_mol * 4, hipMemcpyDeviceToHost));
        for (size_t m = 0; m < n_mol; m++) joff[m + 1] = joff[m] + m_nj[m];
        if (joff[n_mol]) {
            if ((rc = d_jo.put(joff, s)) || (rc = d_jout.alloc(joff[n_mol]))) return rc;
            a.junc_off = d_jo.p;
            a.junc_out = d_jout.p;
            if ((rc = ev.begin(s))) return rc;
            hipLaunchKernelGGL(k_iso<true>, dim3(grid), dim3(64 * kIsoWaves), 0, s, a);
            SMI_HIP(hipGetLastError());
            if ((rc = ev.end(s, &ms[0]))) return rc;
            jset.resize(joff[n_mol]);
            SMI_HIP(hipMemcpy(jset.data(), d_jout.p, jset.size() * 4, hipMemcpyDeviceToHost));
        }
    }
    // molecule gene / transcript ids: a model gene index (or -1 = "undef"), a key id (or -1)
    const auto undef_gene = M.gene_id.find("undef");
    std::vector<int32_t> gid(n_mol);
    for (size_t m = 0; m < n_mol; m++) {
        switch (m_status[m]) {
            case kMono: c[SMI_ISO_MONOEXON]++; break;
            case kOne: c[SMI_ISO_ONEMATCH]++; break;
            case kAmbiguous: c[SMI_ISO_AMBIGUOUS]++; break;
            case kNomatch: c[SMI_ISO_NOMATCH]++; break;
        }
        if (m_key[m] >= 0) {
            auto it = M.gene_id.find(M.key_gene[m_key[m]]);
            gid[m] = it == M.gene_id.end() ? -1 : it->second;
        } else if (m_status[m] == kNomatch) {
            gid[m] = m_gene[m];
        } else {
            gid[m] = undef_gene == M.gene_id.end() ? -2 : undef_gene->second;  // "undef" counts only if it is a model gene
        }
    }
    // counted molecules (produceMatrix / addMolecule): barcode in the cell list, gene in the model
    std::vector<int32_t> cnt_mol, mol_cell(n_mol, -1);
    for (size_t m = 0; m < n_mol; m++) {
        auto it = h->cell_id.find(std::string(sv(h->bc_off, h->bc_len, read_last[mol_first_read[m]])));
        if (it == h->cell_id.end() || gid[m] < 0) continue;
        mol_cell[m] = it->second;
        cnt_mol.push_back((int32_t)m);
    }
    auto bc_of = [&](int32_t m) { return sv(h->bc_off, h->bc_len, read_last[mol_first_read[m]]); };
    auto umi_of = [&](int32_t m) { return sv(h->umi_off, h->umi_len, read_last[mol_first_read[m]]); };
    auto gene_name = [&](int32_t m) { return M.genes[gid[m]]; };
    auto tx_name = [&](int32_t m) { return m_key[m] >= 0 ? M.key_tx[m_key[m]] : std::string("undef"); };
    // rows in byte order of their text: the distinct (gene, key / junction) integer pairs are found first, only their labels are sorted
    auto rows_of = [&](const std::vector<uint64_t> &item, auto label_of, std::vector<std::string> &labels, std::vector<int32_t> &row_of_item) {
        std::vector<uint64_t> u(item);
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
        std::vector<std::string> lab(u.size());
        for (size_t k = 0; k < u.size(); k++) lab[k] = label_of(u[k]);
        std::vector<int32_t> ord(u.size()), rank(u.size());
        for (size_t k = 0; k < u.size(); k++) ord[k] = (int32_t)k;
        std::sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return lab[x] < lab[y]; });
        labels.resize(u.size());
        for (size_t k = 0; k < u.size(); k++) {
            rank[ord[k]] = (int32_t)k;
            labels[k] = std::move(lab[ord[k]]);
        }
        row_of_item.resize(item.size());
        for (size_t i = 0; i < item.size(); i++) row_of_item[i] = rank[std::lower_bound(u.begin(), u.end(), item[i]) - u.begin()];
    };
    auto pair = [](int32_t hi, int32_t lo) { return (uint64_t)(uint32_t)hi << 32 | (uint32_t)(lo + 1); };  // lo -1 (undef) sorts first
    const size_t nc = cnt_mol.size();
    std::vector<std::string> iso_rows, gene_rows, junc_rows;
    std::vector<int32_t> iso_row, gene_row, junc_row;
    std::vector<uint64_t> items(nc);
    for (size_t i = 0; i < nc; i++) items[i] = pair(gid[cnt_mol[i]], m_key[cnt_mol[i]]);
    rows_of(items, [&](uint64_t x) { const int32_t k = (int32_t)(uint32_t)x - 1;
                                     return M.genes[x >> 32] + "\t" + (k >= 0 ? M.key_tx[k] : std::string("undef")); }, iso_rows, iso_row);
    for (size_t i = 0; i < nc; i++) items[i] = pair(gid[cnt_mol[i]], 0);
    rows_of(items, [&](uint64_t x) { return M.genes[x >> 32]; }, gene_rows, gene_row);
    std::vector<int64_t> jitem_mol;
    items.clear();
    for (size_t i = 0; i < nc; i++)
        for (int64_t k = joff[cnt_mol[i]]; k < joff[cnt_mol[i] + 1]; k++) {
            jitem_mol.push_back(cnt_mol[i]);
            items.push_back(pair(gid[cnt_mol[i]], jset[k]));
        }
    rows_of(items, [&](uint64_t x) { const int2 j = M.ujunc[(int32_t)(uint32_t)x - 1];
                                     return M.genes[x >> 32] + ":" + std::to_string(j.x) + "-" + std::to_string(j.y); }, junc_rows, junc_row);
    std::string head;
    for (auto &cell : h->cells) head += "\t" + cell;
    head += "\n";
    std::vector<int64_t> iso_tot, gene_tot, junc_tot;
    std::vector<uint64_t> codes;
    int rc;
    // isoforms
    std::vector<std::string> iso_lab(iso_rows.size());
    std::vector<int32_t> iso_nex(iso_rows.size());
    for (size_t r = 0; r < iso_rows.size(); r++) {
        const size_t tab = iso_rows[r].find('\t');
        const std::string g = iso_rows[r].substr(0, tab), t = iso_rows[r].substr(tab + 1);
        int32_t nex = 0;  // select(gene, tx): the last line of gene g with that transcript
        auto git = M.gene_id.find(g);
        if (git != M.gene_id.end())
            for (int32_t k = M.gene_tx_off[git->second]; k < M.gene_tx_off[git->second + 1]; k++)
                if (M.key_tx[M.tx_key[M.gene_tx[k]]] == t) nex = M.tx_nexon[M.gene_tx[k]];
        iso_nex[r] = nex;
        iso_lab[r] = iso_rows[r] + "\t" + std::to_string(nex);
    }
    codes.resize(nc);
    for (size_t i = 0; i < nc; i++) codes[i] = (uint64_t)iso_row[i] << 32 | (uint32_t)mol_cell[cnt_mol[i]];
    std::string &isom = h->out[SMI_ISO_OUT_ISOMATRIX];
    isom = "geneId\ttranscriptId\tnbExons" + head;
    if ((rc = mtx::matrix(s, "IsoformMatrix", (int32_t)h->cells.size(), h->cfg.budget_bytes, codes, iso_lab, isom, iso_tot, &ms[1], &ms[2],
                          &c[SMI_ISO_RENDER_BLOCKS]))) return rc;
    std::string &isomet = h->out[SMI_ISO_OUT_ISOMETRICS];
    isomet = "geneId\ttranscriptId\tnbExons\tnbUmis\n";
    for (size_t r = 0; r < iso_rows.size(); r++) {
        isomet += iso_lab[r] + "\t" + std::to_string(iso_tot[r]) + "\n";
        c[SMI_ISO_TOTAL_COUNT] += iso_tot[r];
    }
    // genes
    for (size_t i = 0; i < nc; i++) codes[i] = (uint64_t)gene_row[i] << 32 | (uint32_t)mol_cell[cnt_mol[i]];
    codes.resize(nc);
    std::string &genm = h->out[SMI_ISO_OUT_GENEMATRIX];
    genm = "geneId" + head;
    if ((rc = mtx::matrix(s, "IsoformMatrix", (int32_t)h->cells.size(), h->cfg.budget_bytes, codes, gene_rows, genm, gene_tot, &ms[1], &ms[2],
                          &c[SMI_ISO_RENDER_BLOCKS]))) return rc;
    // junctions
    codes.resize(jitem_mol.size());
    for (size_t i = 0; i < jitem_mol.size(); i++) codes[i] = (uint64_t)junc_row[i] << 32 | (uint32_t)mol_cell[jitem_mol[i]];
    std::string &junm = h->out[SMI_ISO_OUT_JUNCMATRIX];
    junm = "junctionId" + head;
    if ((rc = mtx::matrix(s, "IsoformMatrix", (int32_t)h->cells.size(), h->cfg.budget_bytes, codes, junc_rows, junm, junc_tot, &ms[1], &ms[2],
                          &c[SMI_ISO_RENDER_BLOCKS]))) return rc;
    std::string &junmet = h->out[SMI_ISO_OUT_JUNCMETRICS];
    junmet = "junctionId\tnbUmis\n";
    for (size_t r = 0; r < junc_rows.size(); r++) junmet += junc_rows[r] + "\t" + std::to_string(junc_tot[r]) + "\n";
    // gene metrics, cell metrics, molecule infos
    std::vector<int64_t> g_known(gene_rows.size(), 0), g_undef(gene_rows.size(), 0);
    std::vector<int64_t> c_reads(h->cells.size(), 0), c_umis(h->cells.size(), 0), c_known(h->cells.size(), 0), c_undef(h->cells.size(), 0);
    std::vector<std::vector<int32_t>> c_genes(h->cells.size());
    for (size_t i = 0; i < nc; i++) {
        const int32_t m = cnt_mol[i], cell = mol_cell[m];
        const bool undef = m_key[m] < 0;
        (undef ? g_undef : g_known)[gene_row[i]]++;
        (undef ? c_undef : c_known)[cell]++;
        c_umis[cell]++;
        c_reads[cell] += mol_n[m];
        c_genes[cell].push_back(gene_row[i]);
        (undef ? c[SMI_ISO_UNDEF] : c[SMI_ISO_DEF])++;
    }
    std::string &genmet = h->out[SMI_ISO_OUT_GENEMETRICS];
    genmet = "geneId\tnbUmis\tnbIsoformSet\tnbIsoformNotSet\n";
    for (size_t r = 0; r < gene_rows.size(); r++)
        genmet += gene_rows[r] + "\t" + std::to_string(g_known[r] + g_undef[r]) + "\t" + std::to_string(g_known[r]) + "\t" + std::to_string(g_undef[r]) + "\n";
    std::string &cellmet = h->out[SMI_ISO_OUT_CELLMETRICS];
    cellmet = "cellBC\tnbReads\tnbGenes\tnbUmis\tnbIsoformSet\tnbIsoformNotSet\n";
    for (size_t k = 0; k < h->cells.size(); k++) {
        auto &gs = c_genes[k];
        std::sort(gs.begin(), gs.end());
        const size_t ng = std::unique(gs.begin(), gs.end()) - gs.begin();
        cellmet += h->cells[k] + "\t" + std::to_string(c_reads[k]) + "\t" + std::to_string(ng) + "\t" + std::to_string(c_umis[k]) + "\t" +
                   std::to_string(c_known[k]) + "\t" + std::to_string(c_undef[k]) + "\n";
    }
    std::vector<int32_t> mo(cnt_mol);
    std::sort(mo.begin(), mo.end(), [&](int32_t x, int32_t y) {
        const auto bx = bc_of(x), by = bc_of(y);
        return bx != by ? bx < by : umi_of(x) < umi_of(y);
    });
    std::string &mol = h->out[SMI_ISO_OUT_MOLINFOS];
    mol = "cellBC\tUMI\tnbReads\tnbSupportingReads\tmappingPctId\tsnpPhredScore\tgeneId\ttranscriptId\n";
    for (int32_t m : mo) {
        const int32_t rn = h->rn[read_last[mol_first_read[m]]];  // Molecule.rn: the first read's rn (of its last record)
        const int32_t nreads = rn > 1 ? rn : mol_n[m];
        const float pct = 1.0f - h->de[read_first[mol_last_read[m]]];
        mol.append(bc_of(m));
        mol += '\t';
        mol.append(umi_of(m));
        mol += "\t" + std::to_string(nreads) + "\t" + std::to_string(m_support[m]) + "\t" + java_float(pct) + "\t\t" + gene_name(m) + "\t" +
               tx_name(m) + "\n";
    }
    if (h->cfg.to_bulk) {  // writeBulk, with its second loop writing into the bulkgene stream as well
        std::string &bg = h->out[SMI_ISO_OUT_BULKGENE], &bi = h->out[SMI_ISO_OUT_BULKISO];
        bg = "geneId\tcount\n";
        bi = "transcriptId\texons\tcount\n";
        for (size_t r = 0; r < gene_rows.size(); r++) bg += gene_rows[r] + "\t" + std::to_string(gene_tot[r]) + "\n";
        for (size_t r = 0; r < iso_rows.size(); r++) {
            bg += iso_lab[r];
            bi += iso_lab[r] + "\t" + std::to_string(iso_tot[r]) + "\n";
        }
    }
    // ISOBAM's table: "undef" first, then every model gene and every key's transcript
    {
        std::vector<uint64_t> gs(M.genes.size()), ks(M.key_tx.size());
        auto add = [&](const std::string &x) {
            const uint64_t o = h->iso_text.size();
            h->iso_text.insert(h->iso_text.end(), x.begin(), x.end());
            return o;
        };
        add("undef");
        for (size_t g = 0; g < gs.size(); g++) gs[g] = add(M.genes[g]);
        for (size_t k = 0; k < ks.size(); k++) ks[k] = add(M.key_tx[k]);
        h->ig_start.assign(n_mol + 1, 0);
        h->it_start.assign(n_mol + 1, 0);
        h->ig_len.assign(n_mol + 1, 5);
        h->it_len.assign(n_mol + 1, 5);
        for (size_t m = 0; m < n_mol; m++) {
            if (gid[m] >= 0) {
                h->ig_start[m + 1] = gs[gid[m]];
                h->ig_len[m + 1] = (uint32_t)M.genes[gid[m]].size();
            }
            if (m_key[m] >= 0) {
                h->it_start[m + 1] = ks[m_key[m]];
                h->it_len[m + 1] = (uint32_t)M.key_tx[m_key[m]].size();
            }
        }
        h->mol_by_key = std::move(by_key);
    }
    c[SMI_ISO_MATRIX_GENES] = (int64_t)gene_rows.size();
    c[SMI_ISO_MATRIX_JUNCTIONS] = (int64_t)junc_rows.size();
    c[SMI_ISO_MATRIX_ISOFORMS] = (int64_t)iso_rows.size();
    if (stage_ms) std::memcpy(stage_ms, ms, sizeof(ms));
    return SMI_OK;
}

extern "C" int smi_isoform_output(const smi_isoform *h, int32_t which, uint8_t *out, size_t cap, size_t *n_out) {
    if (!h || !n_out || which < 0 || which >= SMI_ISOFORM_OUTPUTS) {
        set_error("smi_isoform_output: bad argument");
        return SMI_ERR_INVALID;
    }
    return handle::get_text(h->out[which], out, cap, n_out);
}

extern "C" int smi_isoform_counts(const smi_isoform *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_isoform_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof(h->counts));
    return SMI_OK;
}

extern "C" int smi_isoform_isobam(smi_isoform *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n, uint8_t *out, size_t cap,
                                  size_t *n_out) {
    if (!h || !n_out || n < 0 || (n && (!bam || !recs))) {
        set_error("smi_isoform_isobam: bad argument");
        return SMI_ERR_INVALID;
    }
    if (!h->ran) {
        set_error("smi_isoform_isobam: the molecules are not assigned yet (smi_isoform_run)");
        return SMI_ERR_STATE;
    }
    *n_out = 0;
    if (!out || !(h->last_n == n && h->last_bam == bam && h->last_recs == recs)) {  // a size query always makes the records
        h->last_n = -1;
        for (int32_t i = 0; i < n; i++) {  // every record inside the buffer, its attributes at its end (K-TAG-ASM reads nothing else)
            const smi_bam_record &r = recs[i];
            if (r.rec_len < 36 || r.rec_off + r.rec_len > n_bam || r.name_off + r.l_read_name > n_bam || r.aux_off < r.rec_off + 36 ||
                r.aux_off + r.aux_len != r.rec_off + r.rec_len) {
                set_error("smi_isoform_isobam: record " + std::to_string(i) + " lies outside the segment");
                return SMI_ERR_INVALID;
            }
        }
        // the lookup key: the raw CELLTAG and UMITAG strings ("null" when absent), as (String) r.getAttribute casts them
        std::vector<int32_t> entry(n > 0 ? n : 1, 0);
        std::vector<int32_t> bad(n > 0 ? n : 1, 0);
        const uint16_t cell_tag = lr::tag16(h->cfg.cell_tag), umi_tag = lr::tag16(h->cfg.umi_tag);
        const int nt = std::max(1, std::min<int>(h->cfg.n_threads, (n + 4095) / 4096));
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++)
            th.emplace_back([&, t] {
                std::string key;
                for (int32_t i = (int32_t)((int64_t)n * t / nt); i < (int32_t)((int64_t)n * (t + 1) / nt); i++) {
                    const uint8_t *p = bam + recs[i].aux_off, *end = p + recs[i].aux_len;
                    lr::Aux cell, umi;
                    while (p < end) {
                        size_t k;
                        if (lr::aux_size(p, end, &k)) {
                            bad[i] = 1;
                            break;
                        }
                        const uint16_t tg = (uint16_t)(p[0] | p[1] << 8);
                        if (tg == cell_tag) cell = lr::Aux{p, k};
                        if (tg == umi_tag) umi = lr::Aux{p, k};
                        p += k;
                    }
                    if (bad[i]) continue;
                    if ((cell.p && cell.p[2] != 'Z') || (umi.p && umi.p[2] != 'Z')) {
                        bad[i] = 2;
                        continue;
                    }
                    key.assign(cell.p ? std::string_view((const char *)cell.p + 3, cell.n - 4) : std::string_view("null"));
                    key += ':';
                    key.append(umi.p ? std::string_view((const char *)umi.p + 3, umi.n - 4) : std::string_view("null"));
                    auto it = h->mol_by_key.find(key);
                    entry[i] = it == h->mol_by_key.end() ? 0 : it->second + 1;
                }
            });
        for (auto &x : th) x.join();
        for (int32_t i = 0; i < n; i++)
            if (bad[i]) {
                const smi_bam_record &r = recs[i];
                set_error("IsoformMatrix: ISOBAM: read " + std::string((const char *)bam + r.name_off, r.l_read_name ? r.l_read_name - 1 : 0) +
                          (bad[i] == 1 ? ": malformed attributes" : ": CELLTAG or UMITAG is not a string"));
                return SMI_ERR_INVALID;
            }
        SMI_HIP(hipSetDevice(h->ctx->device));
        hipStream_t s = h->ctx->stream;
        if (!h->d_iso_text) {
            DevBuf<uint8_t> a{kWho};
            DevBuf<uint64_t> b{kWho}, c2{kWho};
            DevBuf<uint32_t> d{kWho}, e{kWho};
            int rc;
            if ((rc = a.put(h->iso_text, s)) || (rc = b.put(h->ig_start, s)) || (rc = c2.put(h->it_start, s)) || (rc = d.put(h->ig_len, s)) ||
                (rc = e.put(h->it_len, s)))
                return rc;
            SMI_HIP(hipStreamSynchronize(s));
            h->d_iso_text = a.p, a.p = nullptr;
            h->d_ig_start = b.p, b.p = nullptr;
            h->d_it_start = c2.p, c2.p = nullptr;
            h->d_ig_len = d.p, d.p = nullptr;
            h->d_it_len = e.p, e.p = nullptr;
        }
        DevBuf<uint8_t> d_bam{kWho};
        DevBuf<smi_bam_record> d_recs{kWho};
        DevBuf<int32_t> d_entry{kWho};
        int rc;
        if ((rc = d_bam.alloc(n_bam + 1)) || (rc = d_recs.alloc(n)) || (rc = d_entry.put(entry, s))) return rc;
        if (n_bam) SMI_HIP(hipMemcpyAsync(d_bam.p, bam, n_bam, hipMemcpyHostToDevice, s));
        if (n) SMI_HIP(hipMemcpyAsync(d_recs.p, recs, (size_t)n * sizeof(smi_bam_record), hipMemcpyHostToDevice, s));
        if ((rc = tag_assemble_z2(s, d_bam.p, d_recs.p, (size_t)n, d_entry.p, h->d_iso_text, h->d_ig_start, h->d_ig_len, h->d_it_start,
                                  h->d_it_len, "IG", "IT", h->isobam, &h->isobam_ms))) {
            set_error(std::string("IsoformMatrix: ISOBAM: ") + smi_last_error());
            return rc;
        }
        h->last_bam = bam;
        h->last_recs = recs;
        h->last_n = n;
    }
    *n_out = h->isobam.size();
    if (!out) return SMI_OK;
    if (cap < h->isobam.size()) return 1;
    std::memcpy(out, h->isobam.data(), h->isobam.size());
    return SMI_OK;
}
