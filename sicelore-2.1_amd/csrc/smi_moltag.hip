// smi_moltag.hip -- `AddBamMoleculeTags` (org/ipmc/sicelore/programs/AddBamMoleculeTags.java:L38-67), `AddGeneNameTag`
// (AddGeneNameTag.java:L76-160) and `AddBamReadTags` (AddBamReadTags.java:L38-72) on the device: all three read a BAM, decide up to three attributes per record and write every record back in
// input order with those attributes set, replaced or removed.
//   K-NAME  one thread per record: the read name split as Java's String.split does it (L48-57) -> three edits or none; a third piece that
//           is no int is reported through atomicMin of the record index (the first such read of the segment); AddBamReadTags' form of it
//           (k_name_read) splits at '_' into up to four pieces and sets three strings
//   K-GENE  one wavefront per mapped record: alignment blocks from the CIGAR 64 operations per round (wave prefix sum, as K-SNP walks it),
//           the candidate genes of the record's contig by two binary searches over (start, running maximum of end), lanes testing 64 genes
//           at a time, and per candidate the read's locus function and exon hit WITHOUT per-base arrays: lanes hold the blocks of a round,
//           each walks the exons of every transcript from a binary search.  picard's assignLocusFunctionForRange (Gene.java:L151-165) takes
//           the per-base maximum inside block ∩ [txStart, txEnd], getLocusFunction the maximum over bases, blocks and genes, and the
//           ordinals INTERGENIC < INTRONIC < UTR < CODING are also the score order -- so maxima of interval tests give the same value.
//           Records that keep two or more genes are flagged: the ORDER of the names in their value is the reference's HashSet iteration
//           order, which the host's smi_gene_tag_chunk models (gene_tag_chunk_opt is called on exactly those records).
//   K-EDIT  one wavefront per record: k_aux_rewrite<WRITE, EditSource> of smi_auxedit.h, the attribute rewrite shared with K-TAG-ASM
//           (smi_tagbam.hip), as SIZE + exclusive scan + WRITE through an AuxRewriter.  EditSource keeps every record and applies an edit
//           list per record behind its own attributes: set Z from a device byte pool / set integer in htsjdk's smallest type / remove,
//           in order.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "smi_auxedit.h"
#include "smi_handle.h"
#include "smi_internal.h"

namespace smi {
namespace {

constexpr int kGeneWaves = 4;  // waves per block of K-GENE
constexpr int kEdits = 3;      // edits per record
constexpr unsigned long long kNoRecord = ~0ull;

enum : uint8_t { EDIT_NONE = 0, EDIT_SET_Z = 1, EDIT_SET_INT = 2, EDIT_REMOVE = 3 };
struct Edit {
    uint16_t key;  // binary tag
    uint8_t kind;  // EDIT_*
    uint8_t pad;
    uint32_t len;  // SET_Z: payload bytes
    uint64_t src;  // SET_Z: offset in the byte pool
    int64_t val;   // SET_INT
};

// bits of GeneRes.bits
enum : uint8_t { GENE_MAPPED = 1, GENE_KEPT = 2, GENE_MULTI = 4, GENE_SAME = 8, GENE_OPPOSITE = 16, GENE_NO_BLOCK = 32 };
struct GeneRes {
    int32_t gene;  // flat index of the kept gene when exactly one is kept
    uint8_t xf;    // LocusFunction ordinal
    uint8_t bits;
    uint16_t pad;
};

// what K-EDIT applies behind a record's own attributes: its edits in order (SAMRecord.setAttribute in call order: a later edit of a tag wins)
struct EditSource {
    const Edit *edits;    // kEdits per record
    const uint8_t *pool;  // the SET_Z payloads
    struct Tail {
        const Edit *ed;
        __device__ uint32_t put(Field *f, int &n) const {
            for (int k = 0; k < kEdits; k++) {
                const Edit e = ed[k];
                if (e.kind == EDIT_NONE) continue;
                if (e.kind == EDIT_REMOVE) {
                    remove_field(f, n, e.key);
                    continue;
                }
                Field s = {};
                s.key = e.key;
                if (e.kind == EDIT_SET_Z) {
                    s.kind = 3;
                    s.len = e.len;
                    s.src = e.src;
                } else {
                    s.kind = 1;
                    s.ival = e.val;
                    s.type = int_type(e.val);
                }
                if (!put_field(f, n, s)) return SMI_TAG_TOO_MANY_ATTRS;
            }
            return 0;
        }
    };
    __device__ bool keeps(size_t) const { return true; }
    __device__ Tail tail(size_t i) const { return {edits + (size_t)kEdits * i}; }
    __device__ const uint8_t *payload() const { return pool; }
};

// ---- K-NAME ----------------------------------------------------------------------------------------------------------------------------
// String.split(one literal character) of s[0 .. len): the number of pieces (trailing empty pieces dropped, leading and inner ones kept, a
// string without the character one piece, a string of separators only none) and [start, end) of the first MAX in b
template <int MAX>
__device__ int java_split(const uint8_t *s, int len, uint8_t sep, int *b) {
    int last = -1;
    for (int k = 0; k < len; k++)
        if (s[k] != sep) last = k;
    if (last < 0) {
        b[0] = b[1] = 0;
        return len == 0 ? 1 : 0;
    }
    int pieces = 1, start = 0;
    for (int k = 0; k < last; k++)
        if (s[k] == sep) {
            if (pieces <= MAX) {
                b[2 * (pieces - 1)] = start;
                b[2 * (pieces - 1) + 1] = k;
            }
            pieces++;
            start = k + 1;
        }
    if (pieces <= MAX) {
        b[2 * (pieces - 1)] = start;
        b[2 * (pieces - 1) + 1] = last + 1;
    }
    return pieces;
}

__global__ void k_name(const uint8_t *__restrict__ bam, const smi_bam_record *__restrict__ recs, size_t n, uint32_t cell_key, uint32_t umi_key,
                       uint32_t rn_key, Edit *__restrict__ edits, unsigned long long *__restrict__ err_rec, unsigned long long *__restrict__ n_tagged) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    bool tagged = false;
    if (i < n) {
        const smi_bam_record rec = recs[i];
        const uint8_t *s = bam + rec.name_off;
        const int len = rec.l_read_name ? rec.l_read_name - 1 : 0;
        int b[6] = {0, 0, 0, 0, 0, 0};
        int pieces = java_split<3>(s, len, '-', b);            // L49
        if (pieces == 1) pieces = java_split<3>(s, len, '|', b);  // L50-51
        Edit e[kEdits] = {};
        if (pieces == 3) {  // L53-57
            // new Integer(info[2]): an optional sign, decimal digits, the int range, nothing else
            int p = b[4];
            const int q = b[5];
            bool neg = false;
            if (p < q && (s[p] == '-' || s[p] == '+')) neg = s[p++] == '-';
            bool ok = p < q;
            long long x = 0;
            for (; p < q && ok; p++) {
                const uint8_t c = s[p];
                if (c < '0' || c > '9') ok = false;
                else {
                    x = x * 10 + (c - '0');
                    if (x > 2147483648ll) ok = false;
                }
            }
            if (neg) x = -x;
            if (ok && x > 2147483647ll) ok = false;
            if (!ok) atomicMin(err_rec, (unsigned long long)i);  // NumberFormatException: the first such read ends the run
            else {
                tagged = true;
                e[0] = {(uint16_t)cell_key, EDIT_SET_Z, 0, (uint32_t)(b[1] - b[0]), rec.name_off + (uint64_t)b[0], 0};
                e[1] = {(uint16_t)umi_key, EDIT_SET_Z, 0, (uint32_t)(b[3] - b[2]), rec.name_off + (uint64_t)b[2], 0};
                e[2] = {(uint16_t)rn_key, EDIT_SET_INT, 0, 0, 0, x};
            }
        }
        for (int k = 0; k < kEdits; k++) edits[(size_t)kEdits * i + k] = e[k];
    }
    const unsigned long long m = __ballot(tagged);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_tagged, (unsigned long long)__popcll(m));
}

// K-NAME of AddBamReadTags (AddBamReadTags.java:L48-62): the name split at '_'; three pieces are gene, cell, UMI, four pieces carry them
// behind a first piece that is not used; no record stops the program
__global__ void k_name_read(const uint8_t *__restrict__ bam, const smi_bam_record *__restrict__ recs, size_t n, uint32_t gene_key, uint32_t cell_key,
                            uint32_t umi_key, Edit *__restrict__ edits, unsigned long long *__restrict__ n_tagged) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    bool tagged = false;
    if (i < n) {
        const smi_bam_record rec = recs[i];
        const uint8_t *s = bam + rec.name_off;
        const int len = rec.l_read_name ? rec.l_read_name - 1 : 0;
        int b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int pieces = java_split<4>(s, len, '_', b);  // L49
        Edit e[kEdits] = {};
        if (pieces == 3 || pieces == 4) {  // L51-62
            tagged = true;
            const int *p = b + (pieces == 4 ? 2 : 0);
            e[0] = {(uint16_t)gene_key, EDIT_SET_Z, 0, (uint32_t)(p[1] - p[0]), rec.name_off + (uint64_t)p[0], 0};
            e[1] = {(uint16_t)cell_key, EDIT_SET_Z, 0, (uint32_t)(p[3] - p[2]), rec.name_off + (uint64_t)p[2], 0};
            e[2] = {(uint16_t)umi_key, EDIT_SET_Z, 0, (uint32_t)(p[5] - p[4]), rec.name_off + (uint64_t)p[4], 0};
        }
        for (int k = 0; k < kEdits; k++) edits[(size_t)kEdits * i + k] = e[k];
    }
    const unsigned long long m = __ballot(tagged);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_tagged, (unsigned long long)__popcll(m));
}

// ---- K-GENE ----------------------------------------------------------------------------------------------------------------------------
struct GeneArgs {
    const uint8_t *bam;
    const smi_bam_record *recs;
    int n, n_ref;
    const int32_t *contig_off, *g_start, *g_end, *g_runmax, *g_tx_off, *tx, *t_ex_off, *exons;
    const uint8_t *g_neg;
    const uint64_t *name_off;  // [genes + 1] into the pool
    uint64_t sign_off;         // "+-" in the pool
    uint64_t fn_off[4];        // the function names in the pool
    uint32_t fn_len[4];
    uint32_t gene_key, strand_key, fn_key;
    int use_strand, allow_multi;
    Edit *edits;
    GeneRes *res;
    unsigned long long *err_rec;
};

// one round of the CIGAR: lane k0 + lane's operation as a block [bs, be] (is_m) and the reference position behind the round
__device__ __forceinline__ void cigar_round(const GeneArgs &a, const smi_bam_record &r, int k0, int lane, int64_t ref_base, bool &is_m, int64_t &bs,
                                            int64_t &be, int64_t &round_end) {
    const int k = k0 + lane;
    uint32_t c = 0;
    if (k < (int)r.n_cigar) c = ld_u32(a.bam + r.cigar_off + 4ull * k);
    const uint32_t op = c & 15;
    const int64_t len = c >> 4;
    is_m = k < (int)r.n_cigar && (op == 0 || op == 7 || op == 8);   // M = X make a block
    const int64_t rl = (is_m || op == 2 || op == 3) ? len : 0;      // D N advance the reference; I S H P do not
    const int64_t ir = wave_incl_sum(rl, lane);
    bs = ref_base + ir - rl;
    be = bs + len - 1;
    round_end = ref_base + (int64_t)__shfl((long long)ir, 63);
}

__global__ __launch_bounds__(64 * kGeneWaves) void k_gene(GeneArgs a) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kGeneWaves + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const smi_bam_record r = a.recs[i];
    Edit *ed = a.edits + (size_t)kEdits * i;
    if ((r.flag & 4) || r.ref_id < 0) {  // L91: no edit
        if (lane < kEdits) ed[lane] = Edit{};
        if (lane == 0) a.res[i] = GeneRes{-1, 0, 0, 0};
        return;
    }
    // round 0 is kept in registers (most records have fewer than 64 operations); the alignment end needs every round once
    bool m0;
    int64_t bs0, be0, end0;
    const int64_t start = (int64_t)r.pos + 1;
    cigar_round(a, r, 0, lane, start, m0, bs0, be0, end0);
    bool any_block = __ballot(m0) != 0;
    int64_t ref_end = end0;
    for (int k0 = 64; k0 < (int)r.n_cigar; k0 += 64) {
        bool m;
        int64_t bs, be, re;
        cigar_round(a, r, k0, lane, ref_end, m, bs, be, re);
        any_block |= __ballot(m) != 0;
        ref_end = re;
    }
    const int64_t end = ref_end - 1;  // the last reference base consumed
    int xf = 0, n_all = 0, n_same = 0, n_opp = 0, first_all = -1, first_same = -1;
    bool no_block = false;
    const bool neg = (r.flag & 16) != 0;
    if (r.ref_id < a.n_ref) {
        const int g0 = a.contig_off[r.ref_id], g1 = a.contig_off[r.ref_id + 1];
        int lo = g0, hi = g1;  // ub: the first gene that starts behind the alignment
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)a.g_start[mid] <= end) lo = mid + 1;
            else hi = mid;
        }
        const int ub = lo;
        lo = g0, hi = ub;  // lb: the first gene up to which some end reaches the alignment
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)a.g_runmax[mid] < start) lo = mid + 1;
            else hi = mid;
        }
        for (int base = lo; base < ub && !no_block; base += 64) {
            const int gi = base + lane;
            unsigned long long bal = __ballot(gi < ub && (int64_t)a.g_end[gi] >= start);  // [start, end] inclusive at both ends
            if (bal && !any_block) {  // getLocusFunction over a null entry (L362): the reference's loop ends here
                no_block = true;
                break;
            }
            while (bal) {
                const int G = base + (__ffsll((long long)bal) - 1);
                bal &= bal - 1;
                const int t0 = a.g_tx_off[G], t1 = a.g_tx_off[G + 1];
                int f = 0;
                bool hit = false;
                int64_t ref_base = start;
                for (int k0 = 0; k0 < (int)r.n_cigar; k0 += 64) {
                    bool m = m0;
                    int64_t bs = bs0, be = be0, re = end0;
                    if (k0) cigar_round(a, r, k0, lane, ref_base, m, bs, be, re);
                    ref_base = re;
                    if (!m) continue;
                    for (int t = t0; t < t1 && !(f == 3 && hit); t++) {
                        const int32_t *T = a.tx + 4 * (size_t)t;
                        const int64_t cl = max(bs, (int64_t)T[0]), ch = min(be, (int64_t)T[1]);  // block ∩ transcript: the bases assignLocusFunctionForRange visits
                        if (cl <= ch) f = max(f, 1);
                        const int e0 = a.t_ex_off[t], e1 = a.t_ex_off[t + 1];
                        int l = e0, h = e1;  // the first exon that ends at or behind the block's start (exons ascending and disjoint)
                        while (l < h) {
                            const int mid = (l + h) >> 1;
                            if ((int64_t)a.exons[2 * (size_t)mid + 1] < bs) l = mid + 1;
                            else h = mid;
                        }
                        for (int e = l; e < e1; e++) {
                            const int64_t es = a.exons[2 * (size_t)e], ee = a.exons[2 * (size_t)e + 1];
                            if (es > be) break;
                            hit = true;  // getAlignmentBlockOverlapsExon L231-247: the whole block against the whole exon
                            const int64_t xl = max(cl, es), xh = min(ch, ee);
                            if (xl <= xh) f = max(f, max(xl, (int64_t)T[2]) <= min(xh, (int64_t)T[3]) ? 3 : 2);  // some base inside the CDS: CODING, else UTR
                            if (f == 3) break;
                        }
                    }
                }
                for (int o = 32; o > 0; o >>= 1) f = max(f, __shfl_xor(f, o));
                hit = __ballot(hit) != 0;
                xf = max(xf, f);
                if (hit && f >= 2 && a.allow_multi) {  // L126-133; without ALLOW_MULTI_GENE_READS retainAll on the empty set keeps nothing
                    if (!n_all) first_all = G;
                    n_all++;
                    if ((a.g_neg[G] != 0) == neg) {
                        if (!n_same) first_same = G;
                        n_same++;
                    } else
                        n_opp++;
                }
            }
        }
    }
    if (lane) return;
    GeneRes o = {-1, (uint8_t)xf, GENE_MAPPED, 0};
    if (no_block) {
        o.bits |= GENE_NO_BLOCK;
        atomicMin(a.err_rec, (unsigned long long)i);
    }
    const int kept = a.use_strand ? n_same : n_all, first = a.use_strand ? first_same : first_all;
    if (n_same) o.bits |= GENE_SAME;
    if (n_opp) o.bits |= GENE_OPPOSITE;
    if (kept) o.bits |= GENE_KEPT;
    if (kept > 1) o.bits |= GENE_MULTI;
    if (kept == 1) o.gene = first;
    a.res[i] = o;
    ed[0] = {(uint16_t)a.fn_key, EDIT_SET_Z, 0, a.fn_len[xf], a.fn_off[xf], 0};  // L146-147
    if (kept == 1) {                                                           // L149-154
        ed[1] = {(uint16_t)a.gene_key, EDIT_SET_Z, 0, (uint32_t)(a.name_off[first + 1] - a.name_off[first]), a.name_off[first], 0};
        ed[2] = {(uint16_t)a.strand_key, EDIT_SET_Z, 0, 1u, a.sign_off + (a.g_neg[first] ? 1u : 0u), 0};
    } else {  // none kept: both removed (L155-158); two or more: K-GENE-MULTI sets them from the host's ordering
        ed[1] = {(uint16_t)a.gene_key, EDIT_REMOVE, 0, 0, 0, 0};
        ed[2] = {(uint16_t)a.strand_key, EDIT_REMOVE, 0, 0, 0, 0};
    }
}

// the GENETAG / STRANDTAG edits of the records that keep two or more genes, from the values the host ordered
struct MultiPatch {
    int32_t rec;
    uint32_t ge_len, gs_len, pad;
    uint64_t ge_off, gs_off;
};
__global__ void k_gene_multi(const MultiPatch *__restrict__ p, int n, uint32_t gene_key, uint32_t strand_key, Edit *__restrict__ edits) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const MultiPatch x = p[j];
    Edit *ed = edits + (size_t)kEdits * x.rec;
    ed[1] = {(uint16_t)gene_key, EDIT_SET_Z, 0, x.ge_len, x.ge_off, 0};
    ed[2] = {(uint16_t)strand_key, EDIT_SET_Z, 0, x.gs_len, x.gs_off, 0};
}

template <class T>
int upload(T **p, const std::vector<T> &v) {
    SMI_HIP(hipMalloc((void **)p, std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (!v.empty()) SMI_HIP(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return SMI_OK;
}
const char *const kFnName[4] = {"INTERGENIC", "INTRONIC", "UTR", "CODING"};

}  // namespace
}  // namespace smi

using namespace smi;

struct smi_moltag {
    smi_ctx *ctx = nullptr;
    smi_moltag_config cfg = {};
    const smi_genes *genes = nullptr;
    // the gene model on the device (AddGeneNameTag)
    int n_ref = 0;
    size_t n_flat = 0;
    int32_t *d_contig_off = nullptr, *d_g_start = nullptr, *d_g_end = nullptr, *d_g_runmax = nullptr, *d_g_tx_off = nullptr, *d_tx = nullptr,
            *d_t_ex_off = nullptr, *d_exons = nullptr;
    uint8_t *d_g_neg = nullptr;
    uint64_t *d_name_off = nullptr;
    std::vector<uint8_t> pool;  // gene names, "+-", the function names; behind them the multi-gene values of the current segment
    uint64_t sign_off = 0, fn_off[4] = {};
    uint8_t *d_pool = nullptr;
    size_t pool_cap = 0;
    MultiPatch *d_patch = nullptr;
    size_t patch_cap = 0;
    // one segment (grow-only)
    uint8_t *d_bam = nullptr;
    size_t bam_cap = 0;
    smi_bam_record *d_recs = nullptr;
    Edit *d_edits = nullptr;
    GeneRes *d_res = nullptr;
    size_t recs_cap = 0, res_cap = 0, edits_cap = 0;
    AuxRewriter rw;                         // K-EDIT: SIZE + scan, WRITE
    unsigned long long *d_words = nullptr;  // [0] first error record, [1] tagged records
    std::vector<GeneRes> res;
    // the segment the last call sized and did not write: the next call with the same arguments writes it
    const uint8_t *last_bam = nullptr;
    const smi_bam_record *last_recs = nullptr;
    size_t last_n_bam = 0;
    int32_t last_n = -1;
    uint64_t last_total = 0;
    int64_t counts[SMI_MOLTAG_COUNTS] = {};
    std::string error_read;
    int64_t error_record = -1;
    hipEvent_t ev[2] = {};
    float ms[SMI_MOLTAG_STAGES] = {};
};

namespace {

void moltag_release(smi_moltag *h) {
    void *bufs[] = {h->d_contig_off, h->d_g_start, h->d_g_end, h->d_g_runmax, h->d_g_tx_off, h->d_tx, h->d_t_ex_off, h->d_exons, h->d_g_neg, h->d_name_off,
                    h->d_pool, h->d_patch, h->d_bam, h->d_recs, h->d_edits, h->d_res, h->d_words};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
}

// the pool on the device: its fixed part and `extra` bytes behind it
int pool_to_device(smi_moltag *h, hipStream_t s) {
    if (h->pool.size() + 1 > h->pool_cap || !h->d_pool) {
        if (int rc = grow(&h->d_pool, h->pool_cap, h->pool.size() + 1)) return rc;
    }
    SMI_HIP(hipMemcpyAsync(h->d_pool, h->pool.data(), h->pool.size(), hipMemcpyHostToDevice, s));
    return SMI_OK;
}

EditSource edit_source(const smi_moltag *h) { return {h->d_edits, h->cfg.program == SMI_MOLTAG_GENE ? h->d_pool : h->d_bam}; }

}  // namespace

extern "C" int smi_moltag_default_config(int32_t program, smi_moltag_config *cfg) {
    if (!cfg || (program != SMI_MOLTAG_MOLECULE && program != SMI_MOLTAG_GENE && program != SMI_MOLTAG_READ)) {
        set_error("smi_moltag_default_config: bad argument");
        return SMI_ERR_INVALID;
    }
    *cfg = {};
    cfg->program = program;
    std::memcpy(cfg->cell_tag, "BC", 3);
    std::memcpy(cfg->umi_tag, "U8", 3);
    std::memcpy(cfg->rn_tag, "RN", 3);
    std::memcpy(cfg->gene_tag, "GE", 3);
    std::memcpy(cfg->strand_tag, "GS", 3);
    std::memcpy(cfg->function_tag, "XF", 3);
    cfg->use_strand_info = 1;
    cfg->allow_multi_gene_reads = 1;
    return SMI_OK;
}

extern "C" int smi_moltag_create(smi_ctx *ctx, const smi_moltag_config *cfg, const smi_genes *genes, smi_moltag **out) {
    if (!ctx || !cfg || !out) {
        set_error("smi_moltag_create: null argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    const bool gene = cfg->program == SMI_MOLTAG_GENE;
    const bool read = cfg->program == SMI_MOLTAG_READ;
    if (!gene && !read && cfg->program != SMI_MOLTAG_MOLECULE) {
        set_error("smi_moltag_create: unknown program");
        return SMI_ERR_INVALID;
    }
    if (gene && !genes) {
        set_error("smi_moltag_create: AddGeneNameTag needs a gene model");
        return SMI_ERR_INVALID;
    }
    const char *tags[3] = {gene || read ? cfg->gene_tag : cfg->cell_tag, gene ? cfg->strand_tag : read ? cfg->cell_tag : cfg->umi_tag,
                           gene ? cfg->function_tag : read ? cfg->umi_tag : cfg->rn_tag};
    const char *names[3] = {gene || read ? "GENETAG" : "CELLTAG", gene ? "STRANDTAG" : read ? "CELLTAG" : "UMITAG",
                            gene ? "FUNCTIONTAG" : read ? "UMITAG" : "RNTAG"};
    for (int k = 0; k < 3; k++)
        if (!valid_tag(tags[k])) {
            set_error(std::string(names[k]) + " must be two characters");
            return SMI_ERR_INVALID;
        }
    SMI_HIP(hipSetDevice(ctx->device));
    smi_moltag *h = new smi_moltag();
    h->ctx = ctx;
    h->cfg = *cfg;
    h->genes = genes;
    auto fail = [&](int rc) {
        moltag_release(h);
        return rc;
    };
#define MT_TRY(call)                  \
    do {                              \
        if (int rc__ = (call)) return fail(rc__); \
    } while (0)
    for (hipEvent_t &e : h->ev) {
        hipError_t e__ = hipEventCreate(&e);
        if (e__ != hipSuccess) return fail(hip_fail(e__, "hipEventCreate"));
    }
    {
        hipError_t e__ = hipMalloc((void **)&h->d_words, 2 * sizeof(unsigned long long));
        if (e__ != hipSuccess) return fail(hip_fail(e__, "hipMalloc"));
    }
    if (gene) {
        FlatGenes f;
        genes_flatten(genes, f);
        h->n_ref = (int)f.contig_off.size() - 1;
        h->n_flat = f.g_start.size();
        h->counts[SMI_MOLTAG_N_GENES] = (int64_t)f.n_loaded;
        std::vector<uint64_t> name_off;
        for (const std::string &nm : f.g_name) {
            name_off.push_back(h->pool.size());
            h->pool.insert(h->pool.end(), nm.begin(), nm.end());
        }
        name_off.push_back(h->pool.size());
        h->sign_off = h->pool.size();
        h->pool.push_back('+');
        h->pool.push_back('-');
        for (int k = 0; k < 4; k++) {
            h->fn_off[k] = h->pool.size();
            h->pool.insert(h->pool.end(), kFnName[k], kFnName[k] + std::strlen(kFnName[k]));
        }
        MT_TRY(upload(&h->d_contig_off, f.contig_off));
        MT_TRY(upload(&h->d_g_start, f.g_start));
        MT_TRY(upload(&h->d_g_end, f.g_end));
        MT_TRY(upload(&h->d_g_runmax, f.g_runmax));
        MT_TRY(upload(&h->d_g_tx_off, f.g_tx_off));
        MT_TRY(upload(&h->d_tx, f.tx));
        MT_TRY(upload(&h->d_t_ex_off, f.t_ex_off));
        MT_TRY(upload(&h->d_exons, f.exons));
        MT_TRY(upload(&h->d_g_neg, f.g_neg));
        MT_TRY(upload(&h->d_name_off, name_off));
    }
#undef MT_TRY
    *out = h;
    return SMI_OK;
}

extern "C" int smi_moltag_free(smi_moltag *h) {
    if (h) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        moltag_release(h);
    }
    return SMI_OK;
}

extern "C" int smi_moltag_counts(const smi_moltag *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_moltag_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof h->counts);
    return SMI_OK;
}

extern "C" int smi_moltag_stage_ms(const smi_moltag *h, float *ms) {
    if (!h || !ms) {
        set_error("smi_moltag_stage_ms: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(ms, h->ms, sizeof h->ms);
    return SMI_OK;
}

extern "C" int smi_moltag_error_read(const smi_moltag *h, char *name, size_t cap, int64_t *record) {
    if (!h || !record || (cap && !name)) {
        set_error("smi_moltag_error_read: null argument");
        return SMI_ERR_INVALID;
    }
    return handle::error_read(h->error_read, h->error_record, name, cap, record);
}

extern "C" int smi_moltag_segment(smi_moltag *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n, uint8_t *out, size_t cap,
                                  size_t *n_out) {
    if (!h || !n_out || n < 0 || (n && (!bam || !recs))) {
        set_error("smi_moltag_segment: bad argument");
        return SMI_ERR_INVALID;
    }
    *n_out = 0;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    const bool gene = h->cfg.program == SMI_MOLTAG_GENE, read = h->cfg.program == SMI_MOLTAG_READ;
    const bool cached = h->last_n == n && h->last_bam == bam && h->last_recs == recs && h->last_n_bam == n_bam;
    h->last_n = -1;
    uint64_t total = 0;
    if (cached) {
        total = h->last_total;
    } else {
        // every record inside the buffer, its attributes at its end: the kernels read nothing outside bam[0 .. n_bam)
        for (int32_t i = 0; i < n; i++) {
            const smi_bam_record &r = recs[i];
            if (r.rec_len < 36 || r.rec_off + r.rec_len > n_bam || r.name_off < r.rec_off || r.name_off + r.l_read_name > r.rec_off + r.rec_len ||
                r.cigar_off < r.rec_off || r.cigar_off + 4ull * r.n_cigar > r.rec_off + r.rec_len || r.aux_off < r.rec_off + 36 ||
                r.aux_off + r.aux_len != r.rec_off + r.rec_len) {
                set_error("smi_moltag_segment: record index entry " + std::to_string(i) + " points outside the BAM buffer");
                return SMI_ERR_INVALID;
            }
        }
        if (int rc = grow(&h->d_bam, h->bam_cap, n_bam + 1)) return rc;
        if (int rc = grow(&h->d_recs, h->recs_cap, (size_t)n + 1)) return rc;
        if (int rc = grow(&h->d_res, h->res_cap, (size_t)n + 1)) return rc;
        if (int rc = grow(&h->d_edits, h->edits_cap, ((size_t)n + 1) * kEdits)) return rc;
        if (n_bam) SMI_HIP(hipMemcpyAsync(h->d_bam, bam, n_bam, hipMemcpyHostToDevice, s));
        if (n) SMI_HIP(hipMemcpyAsync(h->d_recs, recs, (size_t)n * sizeof(smi_bam_record), hipMemcpyHostToDevice, s));
        SMI_HIP(hipMemsetAsync(h->d_words, 0xFF, 8, s));
        SMI_HIP(hipMemsetAsync(h->d_words + 1, 0, 8, s));
        SMI_HIP(hipEventRecord(h->ev[0], s));
        if (n && read)
            hipLaunchKernelGGL(k_name_read, dim3(blocks_for(n, 256)), dim3(256), 0, s, (const uint8_t *)h->d_bam, (const smi_bam_record *)h->d_recs, (size_t)n,
                               tag_key(h->cfg.gene_tag), tag_key(h->cfg.cell_tag), tag_key(h->cfg.umi_tag), h->d_edits, h->d_words + 1);
        if (n && !gene && !read)
            hipLaunchKernelGGL(k_name, dim3(blocks_for(n, 256)), dim3(256), 0, s, (const uint8_t *)h->d_bam, (const smi_bam_record *)h->d_recs, (size_t)n,
                               tag_key(h->cfg.cell_tag), tag_key(h->cfg.umi_tag), tag_key(h->cfg.rn_tag), h->d_edits, h->d_words, h->d_words + 1);
        if (n && gene) {
            h->pool.resize(h->fn_off[3] + std::strlen(kFnName[3]));  // the fixed part
            if (int rc = pool_to_device(h, s)) return rc;
            GeneArgs a = {};
            a.bam = h->d_bam;
            a.recs = h->d_recs;
            a.n = n;
            a.n_ref = h->n_ref;
            a.contig_off = h->d_contig_off;
            a.g_start = h->d_g_start;
            a.g_end = h->d_g_end;
            a.g_runmax = h->d_g_runmax;
            a.g_tx_off = h->d_g_tx_off;
            a.tx = h->d_tx;
            a.t_ex_off = h->d_t_ex_off;
            a.exons = h->d_exons;
            a.g_neg = h->d_g_neg;
            a.name_off = h->d_name_off;
            a.sign_off = h->sign_off;
            for (int k = 0; k < 4; k++) {
                a.fn_off[k] = h->fn_off[k];
                a.fn_len[k] = (uint32_t)std::strlen(kFnName[k]);
            }
            a.gene_key = tag_key(h->cfg.gene_tag);
            a.strand_key = tag_key(h->cfg.strand_tag);
            a.fn_key = tag_key(h->cfg.function_tag);
            a.use_strand = h->cfg.use_strand_info != 0;
            a.allow_multi = h->cfg.allow_multi_gene_reads != 0;
            a.edits = h->d_edits;
            a.res = h->d_res;
            a.err_rec = h->d_words;
            hipLaunchKernelGGL(k_gene, dim3(blocks_for(n, kGeneWaves)), dim3(64 * kGeneWaves), 0, s, a);
        }
        SMI_HIP(hipGetLastError());
        SMI_HIP(hipEventRecord(h->ev[1], s));
        unsigned long long words[2] = {kNoRecord, 0};
        SMI_HIP(hipMemcpyAsync(words, h->d_words, 16, hipMemcpyDeviceToHost, s));
        h->res.resize((size_t)n + 1);
        if (n && gene) SMI_HIP(hipMemcpyAsync(h->res.data(), h->d_res, (size_t)n * sizeof(GeneRes), hipMemcpyDeviceToHost, s));
        SMI_HIP(hipStreamSynchronize(s));
        h->ms[gene ? 1 : 0] = elapsed(h->ev[0], h->ev[1]);
        if (words[0] != kNoRecord) {  // the reference's loop ends at this record and leaves a cut-off file: the run stops here
            const smi_bam_record &r = recs[words[0]];
            h->error_read.assign((const char *)bam + r.name_off, r.l_read_name ? r.l_read_name - 1u : 0u);
            h->error_record = h->counts[SMI_MOLTAG_RECORDS] + (int64_t)words[0];
            set_error(gene ? "read " + h->error_read + " is mapped without a single M / = / X operation under a gene: its locus function is null "
                                                       "(NullPointerException in AddGeneNameTag.getLocusFunction, AddGeneNameTag.java:L362)"
                           : "read " + h->error_read + ": the third piece of its name is no int (NumberFormatException in AddBamMoleculeTags.java:L56)");
            return 2;
        }
        h->counts[SMI_MOLTAG_RECORDS] += n;
        if (!gene) h->counts[SMI_MOLTAG_TAGGED] += (int64_t)words[1];
        if (gene) {
            std::vector<int32_t> multi;
            int64_t mapped = 0, wrong = 0, right = 0, fixed = 0, with_gene = 0;
            for (int32_t i = 0; i < n; i++) {
                const uint8_t b = h->res[(size_t)i].bits;
                if (!(b & GENE_MAPPED)) continue;
                mapped++;
                if (b & GENE_KEPT) with_gene++;
                if (b & GENE_MULTI) multi.push_back(i);
                if (!(b & GENE_SAME) && (b & GENE_OPPOSITE)) wrong++;  // L178-181
                else {
                    if (b & GENE_OPPOSITE) fixed++;  // L188-190
                    right++;                          // L191: also a record with no gene at all
                }
            }
            h->counts[SMI_MOLTAG_TAGGED] += mapped;
            h->counts[SMI_MOLTAG_WITH_GENE] += with_gene;
            h->counts[SMI_MOLTAG_MULTI_GENE] += (int64_t)multi.size();
            if (h->cfg.use_strand_info) {  // the counters are ints in the reference (ReadTaggingMetric L399-403)
                h->counts[SMI_MOLTAG_TOTAL_READS] = (int32_t)(h->counts[SMI_MOLTAG_TOTAL_READS] + mapped);
                h->counts[SMI_MOLTAG_WRONG_STRAND] = (int32_t)(h->counts[SMI_MOLTAG_WRONG_STRAND] + wrong);
                h->counts[SMI_MOLTAG_RIGHT_STRAND] = (int32_t)(h->counts[SMI_MOLTAG_RIGHT_STRAND] + right);
                h->counts[SMI_MOLTAG_AMBIGUOUS_FIXED] = (int32_t)(h->counts[SMI_MOLTAG_AMBIGUOUS_FIXED] + fixed);
            }
            if (!multi.empty()) {  // the order of the names in a multi-gene value: the host's model of the HashSet iteration, on these records only
                const size_t m = multi.size();
                std::vector<int32_t> rid(m), p0(m);
                std::vector<uint16_t> fl(m);
                std::vector<uint32_t> coff(m + 1, 0), cg;
                for (size_t j = 0; j < m; j++) {
                    const smi_bam_record &r = recs[multi[j]];
                    rid[j] = r.ref_id;
                    p0[j] = r.pos;
                    fl[j] = r.flag;
                    const size_t at = cg.size();
                    cg.resize(at + r.n_cigar);
                    if (r.n_cigar) std::memcpy(cg.data() + at, bam + r.cigar_off, 4ull * r.n_cigar);
                    coff[j + 1] = (uint32_t)cg.size();
                }
                if (cg.empty()) cg.push_back(0);
                std::vector<uint32_t> off(3 * m + 1);
                size_t need = 0;
                if (int rc = gene_tag_chunk_opt(h->genes, rid.data(), fl.data(), p0.data(), cg.data(), coff.data(), (int32_t)m, h->cfg.use_strand_info != 0,
                                                nullptr, 0, off.data(), &need))
                    return rc;
                const size_t base = h->pool.size();
                h->pool.resize(base + need + 1);
                if (int rc = gene_tag_chunk_opt(h->genes, rid.data(), fl.data(), p0.data(), cg.data(), coff.data(), (int32_t)m, h->cfg.use_strand_info != 0,
                                                (char *)h->pool.data() + base, need, off.data(), &need))
                    return rc;
                std::vector<MultiPatch> patch(m);
                for (size_t j = 0; j < m; j++) {
                    patch[j] = {multi[j], off[3 * j + 1] - off[3 * j], off[3 * j + 2] - off[3 * j + 1], 0, base + off[3 * j], base + off[3 * j + 1]};
                    if (!std::memchr(h->pool.data() + base + off[3 * j], ',', patch[j].ge_len)) {
                        set_error("smi_moltag_segment: K-GENE and the host's gene tagger disagree on a multi-gene record (internal error)");
                        return SMI_ERR_INVALID;
                    }
                }
                if (int rc = pool_to_device(h, s)) return rc;
                if (int rc = grow(&h->d_patch, h->patch_cap, m)) return rc;
                SMI_HIP(hipMemcpyAsync(h->d_patch, patch.data(), m * sizeof(MultiPatch), hipMemcpyHostToDevice, s));
                hipLaunchKernelGGL(k_gene_multi, dim3(blocks_for(m, 256)), dim3(256), 0, s, (const MultiPatch *)h->d_patch, (int)m,
                                   tag_key(h->cfg.gene_tag), tag_key(h->cfg.strand_tag), h->d_edits);
                SMI_HIP(hipGetLastError());
                SMI_HIP(hipStreamSynchronize(s));  // patch is read by the copy above
            }
        }
        if (int rc = h->rw.size("smi_moltag_segment: ", s, h->d_bam, h->d_recs, (size_t)n, edit_source(h), &total, &h->ms[2])) return rc;
    }
    *n_out = total;
    if (!out || cap < total) {  // sizes only: the segment stays on the device for the next call with the same arguments
        h->last_bam = bam;
        h->last_recs = recs;
        h->last_n_bam = n_bam;
        h->last_n = n;
        h->last_total = total;
        return out ? 1 : SMI_OK;
    }
    if (!total) return SMI_OK;
    return h->rw.write("smi_moltag_segment: ", s, h->d_bam, h->d_recs, (size_t)n, edit_source(h), total, out, &h->ms[3]);
}
