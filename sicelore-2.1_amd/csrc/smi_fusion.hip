// smi_fusion.hip -- `FusionDetector` (org/ipmc/sicelore/programs/FusionDetector.java:L54-113, the reference README's step 6, "Fusion
// transcripts detection cell by cell"): the molecules of a tagged BAM whose reads name exactly two genes, counted per cell.  The rules are
// DESIGN.md section 8i's; tests/fusionmodel.py implements the same ones.
//
// Host (smi_fusion_add_segment), per segment on host threads: LongreadRecord.fromSAMRecord L71-184 and LongreadParser.parseSAMRecord
//   L96-115 with the parameters of FusionDetector.java L63-67 (tags BC U8 GE RN, MAXCLIP 10000, gene mandatory, UMI not, mapq-0 records
//   kept when primary).  Of every kept record, in file order, the read name, the barcode ("-1" removed), the UMI or that it has none, rn,
//   de and the fields of GE.split(",") (Longread.addRecord L40-54) go to pools that live across segments.
// Device (smi_fusion_run): every group is a group of equal byte strings; no host map takes part.
//   K-FUS-INSERT: one kernel over a byte pool and an offset table, used for the read names, the molecule keys, the gene names and the cell
//     list.  Open addressing over a table of a power of two >= 2 x keys (or 2^table_log2), 64-bit FNV-1a of the bytes, walked by probe()
//     of smi_device.h: a key claims an empty slot by CAS of its index, or joins the slot's representative when length and bytes of the
//     two keys are equal, or probes on, wrapping at the end.  Which key of a group becomes its representative is a race: the group's accumulators are indexed by it, every
//     one of them is an atomicMin / atomicMax / integer atomicAdd over record numbers, and groups are renumbered by their smallest member,
//     so nothing that leaves the device depends on it.  The look-up form of the same kernel answers the cell list's contains().
//   K-FUS-READ: LongreadParser L61-79 and Longread.addRecord per read group: its first kept record (atomicMin), its last record
//     (atomicMax: barcode, rn), its last record with a UMI (atomicMax over those); reads are numbered by their first record, and the
//     read's molecule key is written: barcode, ':', UMI, and one byte that tells a missing UMI from any text (MoleculeDataset L76).
//   K-FUS-MOL: MoleculeDataset L69-84 with Molecule.addLongread L127-135: reads per molecule, its first read (the constructor's barcode,
//     UMI and rn) and its last read (pctId = 1 - de of that read's first record); molecules are numbered by their first read.
//   K-FUS-GENES: one (molecule << 32 | gene) code per gene field, the gene numbered by the first field that holds its name; hipcub radix
//     sort + run-length encoding; distinct genes per molecule; the selection of FusionDetector.java L81 (listed cell, a UMI, two genes);
//     the two names in the order a java.util.HashSet of 16 buckets iterates them (bucket (h ^ h >>> 16) & 15 of String.hashCode, computed
//     from the bytes; a shared bucket: byte order); the ordered pairs sorted and run-length encoded once more, which numbers them.
// Host again: the label of every pair (L82-85), the labels sorted; K-MTX (smi_mtx.h) renders the matrix from one (row << 32 | cell) code
//   per counted molecule and gives the row totals of the metrics; the molinfos text (Matrix.writeIsoformMatrix L209-214).
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "smi_device.h"
#include "smi_handle.h"
#include "smi_internal.h"
#include "smi_mtx.h"

namespace smi {
namespace {


constexpr const char *kWho = "FusionDetector";  // the program named when a device allocation fails

constexpr int kFusBlock = 256;
constexpr uint64_t kNoPair = ~0ull;
constexpr int32_t kMaxClip = 10000;  // FusionDetector.java L64

// keys back to back in a pool: key i is pool[off[i] .. off[i + 1])
struct Keys {
    const uint8_t *pool;
    const uint64_t *off;
};

__device__ __forceinline__ Bytes key_bytes(const Keys &k, uint32_t i) {
    const uint64_t o = k.off[i];
    return {k.pool + o, (uint32_t)(k.off[i + 1] - o)};
}

// K-FUS-INSERT.  INSERT: key i of `keys` -> group[i] = the representative of its group (a key index), -1 if the table is full (*overflow
// set).  LOOKUP: key idx[i] of `query` is looked up among the keys of a finished table -> group[i] = the entry that equals it, or -1.
struct InsArgs {
    Keys keys;           // what the table's entries index
    Keys query;          // LOOKUP only
    const int32_t *idx;  // LOOKUP only: the query key of i
    uint32_t n, mask;
    uint32_t *tab;
    int32_t *group;
    unsigned long long *probe_steps, *wraps;
    uint32_t *overflow;
};

template <bool LOOKUP>
__global__ __launch_bounds__(kFusBlock) void k_fus_insert(InsArgs a) {
    const uint32_t i = blockIdx.x * kFusBlock + threadIdx.x;
    if (i >= a.n) return;
    const Keys &mk = LOOKUP ? a.query : a.keys;
    const uint32_t me = LOOKUP ? (uint32_t)a.idx[i] : i;
    const Bytes mine = key_bytes(mk, me);
    const uint64_t h = fnv1a(mine.p, mine.n);
    const Keys keys = a.keys;
    const Probed r = probe<!LOOKUP>(a.tab, a.mask, (uint32_t)(h ^ (h >> 32)) & a.mask, i, mine, [keys](uint32_t e) { return key_bytes(keys, e); });
    a.group[i] = (int32_t)r.entry;  // kEmpty is -1
    if (!LOOKUP && r.entry == kEmpty) atomicOr(a.overflow, 1u);
    if (r.steps) atomicAdd(a.probe_steps, (unsigned long long)r.steps);
    if (r.wraps) atomicAdd(a.wraps, (unsigned long long)r.wraps);
}

// lo[i] = INT_MAX, hi[i] = hi2[i] = -1, cnt[i] = 0 (a null array is left out)
__global__ __launch_bounds__(kFusBlock) void k_fus_init(int32_t *lo, int32_t *hi, int32_t *hi2, int32_t *cnt, int32_t n) {
    const int i = blockIdx.x * kFusBlock + threadIdx.x;
    if (i >= n) return;
    if (lo) lo[i] = INT_MAX;
    if (hi) hi[i] = -1;
    if (hi2) hi2[i] = -1;
    if (cnt) cnt[i] = 0;
}

// K-FUS-READ, the reductions: per read group (indexed by its representative record) over the record numbers, which are in file order
__global__ __launch_bounds__(kFusBlock) void k_fus_read(const int32_t *__restrict__ rep, const uint8_t *__restrict__ has_umi, int32_t n, int32_t *first,
                                                        int32_t *last, int32_t *last_umi, int32_t *nrec) {
    const int r = blockIdx.x * kFusBlock + threadIdx.x;
    if (r >= n) return;
    const int g = rep[r];
    atomicMin(&first[g], r);
    atomicMax(&last[g], r);
    if (has_umi[r]) atomicMax(&last_umi[g], r);
    atomicAdd(&nrec[g], 1);
}

// flag[i] = 1 where element i is the smallest member of its group (n + 1 entries, the last one 0: the scan's total)
__global__ __launch_bounds__(kFusBlock) void k_fus_flag(const int32_t *__restrict__ rep, const int32_t *__restrict__ first, int32_t n, int32_t *flag) {
    const int i = blockIdx.x * kFusBlock + threadIdx.x;
    if (i > n) return;
    flag[i] = i < n && first[rep[i]] == i;
}

// K-FUS-READ, the reads: read q (numbered by first record) of first record r: its last record (barcode, rn), its last record with a UMI
// (-1: none), the bytes of its molecule key; *n_multi counts the reads of more than one record (multiRec, LongreadParser L72)
struct ReadArgs {
    const int32_t *rep, *flag, *rq;  // per record: group, 1 = first record of its read, reads in front of it
    const int32_t *last, *last_umi, *nrec;
    const uint64_t *bc_off, *umi_off;
    int32_t n;
    int32_t *q_first, *q_last, *q_umi;
    uint64_t *klen;
    unsigned long long *n_multi;
};

__global__ __launch_bounds__(kFusBlock) void k_fus_read_list(ReadArgs a) {
    const int r = blockIdx.x * kFusBlock + threadIdx.x;
    bool multi = false;
    if (r < a.n && a.flag[r]) {
        const int g = a.rep[r], q = a.rq[r], l = a.last[g], u = a.last_umi[g];
        a.q_first[q] = r;
        a.q_last[q] = l;
        a.q_umi[q] = u;
        a.klen[q] = (a.bc_off[l + 1] - a.bc_off[l]) + 1 + (u >= 0 ? a.umi_off[u + 1] - a.umi_off[u] : 0) + 1;
        multi = a.nrec[g] > 1;
    }
    const unsigned long long bal = __ballot(multi);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(a.n_multi, (unsigned long long)__popcll(bal));
}

__global__ __launch_bounds__(kFusBlock) void k_fus_read_key(const int32_t *__restrict__ q_last, const int32_t *__restrict__ q_umi, int32_t n_reads,
                                                            const uint8_t *__restrict__ bc, const uint64_t *__restrict__ bc_off,
                                                            const uint8_t *__restrict__ umi, const uint64_t *__restrict__ umi_off,
                                                            const uint64_t *__restrict__ koff, uint8_t *__restrict__ key) {
    const int q = blockIdx.x * kFusBlock + threadIdx.x;
    if (q >= n_reads) return;
    const int l = q_last[q], u = q_umi[q];
    uint8_t *dst = key + koff[q];
    uint64_t k = 0;
    for (uint64_t b = bc_off[l]; b < bc_off[l + 1]; b++) dst[k++] = bc[b];
    dst[k++] = ':';
    if (u >= 0)
        for (uint64_t b = umi_off[u]; b < umi_off[u + 1]; b++) dst[k++] = umi[b];
    dst[k] = u >= 0 ? 1 : 0;
}

// K-FUS-MOL, the reductions: per molecule group (indexed by its representative read) over the read numbers
__global__ __launch_bounds__(kFusBlock) void k_fus_mol(const int32_t *__restrict__ mrep, int32_t n_reads, int32_t *m_first, int32_t *m_last, int32_t *m_n) {
    const int q = blockIdx.x * kFusBlock + threadIdx.x;
    if (q >= n_reads) return;
    const int g = mrep[q];
    atomicMin(&m_first[g], q);
    atomicMax(&m_last[g], q);
    atomicAdd(&m_n[g], 1);
}

// K-FUS-MOL, the molecules: molecule j (numbered by first read): reads, the records its barcode, UMI, rn and de come from
struct MolArgs {
    const int32_t *mrep, *mflag, *mq;  // per read: group, 1 = first read of its molecule, molecules in front of it
    const int32_t *m_first, *m_last, *m_n;
    const int32_t *q_first, *q_last, *q_umi;
    int32_t n_reads;
    int32_t *read_mol;                             // per read
    int32_t *mol_n, *mol_bc, *mol_umi, *mol_de;    // per molecule: reads; record of the barcode and rn, of the UMI (-1 none), of de
};

__global__ __launch_bounds__(kFusBlock) void k_fus_mol_list(MolArgs a) {
    const int q = blockIdx.x * kFusBlock + threadIdx.x;
    if (q >= a.n_reads) return;
    const int g = a.mrep[q], j = a.mq[a.m_first[g]];
    a.read_mol[q] = j;
    if (!a.mflag[q]) return;
    a.mol_n[j] = a.m_n[g];
    a.mol_bc[j] = a.q_last[q];               // new Molecule(lr.getBarcode(), lr.getUmi(), lr.getRn()) of the first read
    a.mol_umi[j] = a.q_umi[q];
    a.mol_de[j] = a.q_first[a.m_last[g]];    // getLongreadrecords().get(0) of the read added last
}

// K-FUS-GENES 1: the gene of a field = the first field with that name; one code per field
__global__ __launch_bounds__(kFusBlock) void k_fus_gene_first(const int32_t *__restrict__ grep, int32_t n_fields, int32_t *g_first) {
    const int f = blockIdx.x * kFusBlock + threadIdx.x;
    if (f < n_fields) atomicMin(&g_first[grep[f]], f);
}

struct CodeArgs {
    const int32_t *grep, *g_first, *f_rec;  // per field: group, (per group) first field, its record
    const int32_t *rep, *first, *rq, *read_mol;
    int32_t n_fields;
    uint64_t *code;
    unsigned long long *n_genes;
};

__global__ __launch_bounds__(kFusBlock) void k_fus_codes(CodeArgs a) {
    const int f = blockIdx.x * kFusBlock + threadIdx.x;
    bool is_first = false;
    if (f < a.n_fields) {
        const int g = a.g_first[a.grep[f]], r = a.f_rec[f];
        const int j = a.read_mol[a.rq[a.first[a.rep[r]]]];
        a.code[f] = (uint64_t)(uint32_t)j << 32 | (uint32_t)g;
        is_first = g == f;
    }
    const unsigned long long bal = __ballot(is_first);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(a.n_genes, (unsigned long long)__popcll(bal));
}

// K-FUS-GENES 3: one distinct code = one gene of that molecule; the molecule's codes are a run that starts at g_start
__global__ __launch_bounds__(kFusBlock) void k_fus_gene_count(const uint64_t *__restrict__ ucode, const int64_t *__restrict__ n_run, int32_t *mol_ng,
                                                              int32_t *mol_gstart) {
    const int64_t k = blockIdx.x * (int64_t)kFusBlock + threadIdx.x;
    if (k >= *n_run) return;
    const uint32_t j = (uint32_t)(ucode[k] >> 32);
    atomicAdd(&mol_ng[j], 1);
    if (k == 0 || (uint32_t)(ucode[k - 1] >> 32) != j) mol_gstart[j] = (int32_t)k;
}

// HashMap.hash(String.hashCode()) & 15 over the bytes of a name
__device__ __forceinline__ uint32_t java_bucket(const uint8_t *__restrict__ p, uint32_t n) {
    uint32_t h = 0;
    for (uint32_t k = 0; k < n; k++) h = 31u * h + p[k];
    return (h ^ (h >> 16)) & 15u;
}

// K-FUS-GENES 4, 5: the selection of FusionDetector.java L81 and the pair in the set's iteration order
struct SelArgs {
    const int32_t *mol_ng, *mol_gstart, *mol_umi, *mol_cell;
    const uint64_t *ucode;
    Keys genes;
    int32_t n_mol;
    uint64_t *pair;
    unsigned long long *n_multi_ig;
};

__global__ __launch_bounds__(kFusBlock) void k_fus_select(SelArgs a) {
    const int j = blockIdx.x * kFusBlock + threadIdx.x;
    bool multi = false;
    if (j < a.n_mol) {
        const int ng = a.mol_ng[j];
        multi = ng > 1;
        uint64_t pr = kNoPair;
        if (ng == 2 && a.mol_cell[j] >= 0 && a.mol_umi[j] >= 0) {
            const int s = a.mol_gstart[j];
            uint32_t g0 = (uint32_t)a.ucode[s], g1 = (uint32_t)a.ucode[s + 1];
            const uint8_t *p0 = a.genes.pool + a.genes.off[g0], *p1 = a.genes.pool + a.genes.off[g1];
            const uint32_t n0 = (uint32_t)(a.genes.off[g0 + 1] - a.genes.off[g0]), n1 = (uint32_t)(a.genes.off[g1 + 1] - a.genes.off[g1]);
            const uint32_t b0 = java_bucket(p0, n0), b1 = java_bucket(p1, n1);
            bool swap = b1 < b0;
            if (b0 == b1) {  // byte order: the first byte that differs, else the shorter name
                const uint32_t m = min(n0, n1);
                uint32_t k = 0;
                while (k < m && p0[k] == p1[k]) k++;
                swap = k < m ? p1[k] < p0[k] : n1 < n0;
            }
            if (swap) {
                const uint32_t t = g0;
                g0 = g1;
                g1 = t;
            }
            pr = (uint64_t)g0 << 32 | g1;
        }
        a.pair[j] = pr;
    }
    const unsigned long long bal = __ballot(multi);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(a.n_multi_ig, (unsigned long long)__popcll(bal));
}

// K-FUS-GENES 6: the number of a molecule's pair among the distinct pairs (sorted), -1 for a molecule that is not counted
__global__ __launch_bounds__(kFusBlock) void k_fus_pair_id(const uint64_t *__restrict__ pair, int32_t n_mol, const uint64_t *__restrict__ upair,
                                                           const int64_t *__restrict__ n_run, int32_t *mol_pair) {
    const int j = blockIdx.x * kFusBlock + threadIdx.x;
    if (j >= n_mol) return;
    const uint64_t p = pair[j];
    int32_t id = -1;
    if (p != kNoPair) {
        int64_t lo = 0, hi = *n_run - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (upair[mid] < p) lo = mid + 1;
            else hi = mid;
        }
        id = (int32_t)lo;
    }
    mol_pair[j] = id;
}

inline unsigned grid(size_t n) { return (unsigned)((n + kFusBlock - 1) / kFusBlock); }

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// strings back to back: string i is pool[off[i] .. off[i + 1])
struct Pool {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off{0};
    void add(std::string_view v) {
        bytes.insert(bytes.end(), v.begin(), v.end());
        off.push_back(bytes.size());
    }
    size_t size() const { return off.size() - 1; }
    std::string_view at(size_t i) const { return std::string_view((const char *)bytes.data() + off[i], off[i + 1] - off[i]); }
};

// String.replace(target, with): every occurrence, left to right
std::string jreplace(std::string s, const std::string &target, const std::string &with) {
    for (size_t k = s.find(target); k != std::string::npos; k = s.find(target, k + with.size())) s.replace(k, target.size(), with);
    return s;
}

uint32_t java_bucket_host(std::string_view s) {
    uint32_t h = 0;
    for (unsigned char c : s) h = 31u * h + c;
    return (h ^ (h >> 16)) & 15u;
}

}  // namespace
}  // namespace smi

using namespace smi;

struct smi_fusion {
    smi_ctx *ctx = nullptr;
    smi_fusion_config cfg = {};
    Pool cells;  // the cell list: distinct, in byte order
    // kept records in file order
    Pool names, bcs, umis, genes;  // genes: one entry per gene field
    std::vector<uint8_t> has_umi;
    std::vector<int32_t> rn, f_rec, f_start{0};  // f_rec: the record of a field; f_start: the fields of a record
    std::vector<float> de;
    int64_t counts[SMI_FUSION_COUNTS] = {};
    std::string out[SMI_FUSION_OUTPUTS];
    std::string error_read;
    int64_t error_record = -1;
    int64_t seen = 0;
    bool ran = false, failed = false;
    // the device's result per molecule, kept for smi_fusion_host_loop
    std::vector<int32_t> k_ng;
    std::vector<uint64_t> k_pair;
};

extern "C" int smi_fusion_default_config(smi_fusion_config *cfg) {
    if (!cfg) {
        set_error("smi_fusion_default_config: null argument");
        return SMI_ERR_INVALID;
    }
    *cfg = {};
    cfg->n_threads = 4;
    return SMI_OK;
}

extern "C" int smi_fusion_create(smi_ctx *ctx, const smi_fusion_config *cfg, const char *csv, size_t n_csv, smi_fusion **out) {
    if (!ctx || !cfg || !out || (n_csv && !csv)) {
        set_error("smi_fusion_create: null argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    if (cfg->table_log2 < 0 || cfg->table_log2 > 31) {
        set_error("smi_fusion_config.table_log2 must be 0 .. 31");
        return SMI_ERR_INVALID;
    }
    smi_fusion *h = new smi_fusion();
    h->ctx = ctx;
    h->cfg = *cfg;
    h->cfg.n_threads = std::max(1, std::min(cfg->n_threads, 256));
    std::vector<std::string> cells = handle::cell_list(csv, n_csv);
    std::sort(cells.begin(), cells.end());
    cells.erase(std::unique(cells.begin(), cells.end()), cells.end());
    for (auto &c : cells) h->cells.add(c);
    h->counts[SMI_FUS_CELLS] = (int64_t)cells.size();
    *out = h;
    return SMI_OK;
}

extern "C" int smi_fusion_free(smi_fusion *h) {
    delete h;
    return SMI_OK;
}

extern "C" int smi_fusion_error_read(const smi_fusion *h, char *name, size_t cap, int64_t *record) {
    if (!h || !record || (cap && !name)) {
        set_error("smi_fusion_error_read: null argument");
        return SMI_ERR_INVALID;
    }
    return handle::error_read(h->error_read, h->error_record, name, cap, record);
}

extern "C" int smi_fusion_counts(const smi_fusion *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_fusion_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof h->counts);
    return SMI_OK;
}

extern "C" int smi_fusion_output(const smi_fusion *h, int32_t which, uint8_t *out, size_t cap, size_t *n_out) {
    if (!h || !n_out || which < 0 || which >= SMI_FUSION_OUTPUTS) {
        set_error("smi_fusion_output: bad argument");
        return SMI_ERR_INVALID;
    }
    return handle::get_text(h->out[which], out, cap, n_out);
}

extern "C" int smi_fusion_add_segment(smi_fusion *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n) {
    if (!h || n < 0 || (n && (!bam || !recs))) {
        set_error("smi_fusion_add_segment: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->ran || h->failed) {
        set_error(h->ran ? "smi_fusion_add_segment: the fusions were already detected (smi_fusion_run)" : "smi_fusion_add_segment: an earlier segment failed");
        return SMI_ERR_STATE;
    }
    static const lr::TagSet tags = lr::TagSet().set(lr::kCell, "BC").set(lr::kUmi, "U8").set(lr::kGene, "GE").set(lr::kRn, "RN");  // L63-67
    const lr::Segment seg = lr::read_segment("smi_fusion_add_segment", bam, n_bam, recs, n, h->cfg.n_threads,
                                             [&](const uint8_t *b, const smi_bam_record &r, lr::Record &out, std::string &err) { lr::read_fusion(b, r, tags, kMaxClip, out, err); });
    if (!seg.refused.empty()) {
        set_error(seg.refused);
        return SMI_ERR_INVALID;
    }
    if (seg.first_error >= 0) {
        h->failed = true;
        h->error_read = std::string(lr::read_name(bam, recs[seg.first_error]));
        h->error_record = h->seen + seg.first_error;
        set_error("FusionDetector: read " + h->error_read + ": " + seg.error);
        return SMI_ERR_INVALID;
    }
    // GE.split(",") of Longread.addRecord L40-54.  jsplit("") is one empty field, which addRecord never sees: a kept record's gene is
    // never empty (read_fusion tests no_gene).
    std::vector<std::string_view> fields;
    size_t add_rec = 0, add_fields = 0;
    for (const lr::Record &p : seg.recs) {
        if (p.what != lr::kKept) continue;
        lr::jsplit(p.gene, ',', fields);
        add_rec++;
        add_fields += fields.size();
    }
    // records, reads, molecules and gene fields are numbered in int32 from here on (the kernels' indices, the hipcub calls)
    if (h->names.size() + add_rec > (size_t)INT32_MAX || h->genes.size() + add_fields > (size_t)INT32_MAX) {
        h->failed = true;
        set_error("FusionDetector: more than 2^31 - 1 kept records or gene fields in one run");
        return SMI_ERR_INVALID;
    }
    int64_t *c = h->counts;
    for (int32_t i = 0; i < n; i++) {
        const lr::Record &p = seg.recs[i];
        c[SMI_FUS_RECORDS]++;
        if (p.what != lr::kKept) {
            c[SMI_FUS_UNVALID]++;
            c[p.what == lr::kNull ? SMI_FUS_NULL : p.what == lr::kChimeric ? SMI_FUS_CHIMERIA : p.what == lr::kNoGene ? SMI_FUS_NO_GENE : SMI_FUS_MAPQV0]++;
            continue;
        }
        c[SMI_FUS_VALID]++;
        const int32_t r = (int32_t)h->names.size();
        h->names.add(lr::read_name(bam, recs[i]));
        h->bcs.add(lr::drop_minus1(p.bc));  // L83
        h->umis.add(p.has_umi ? p.umi : std::string_view());
        h->has_umi.push_back(p.has_umi);
        h->rn.push_back(p.rn);
        h->de.push_back(p.de);
        lr::jsplit(p.gene, ',', fields);
        for (auto f : fields) {
            h->genes.add(f);
            h->f_rec.push_back(r);
        }
        h->f_start.push_back((int32_t)h->genes.size());
    }
    h->seen += n;
    return SMI_OK;
}

namespace smi {
namespace {

int table_size(const smi_fusion *h, size_t n, const char *what, uint32_t *mask) {
    uint64_t size = 2;
    if (h->cfg.table_log2) {
        size = 1ull << h->cfg.table_log2;
        if (size < n) {
            set_error("FusionDetector: table_log2 " + std::to_string(h->cfg.table_log2) + " gives a table of fewer slots than the " + std::to_string(n) +
                      " " + what);
            return SMI_ERR_INVALID;
        }
    } else {
        while (size < 2 * (uint64_t)n) size <<= 1;
    }
    *mask = (uint32_t)(size - 1);
    return SMI_OK;
}

}  // namespace
}  // namespace smi

extern "C" int smi_fusion_run(smi_fusion *h, float *stage_ms) {
    if (!h) {
        set_error("smi_fusion_run: null argument");
        return SMI_ERR_INVALID;
    }
    float ms[SMI_FUSION_STAGES] = {};
    if (stage_ms) std::memset(stage_ms, 0, sizeof(ms));
    if (h->ran || h->failed) {
        set_error(h->ran ? "smi_fusion_run: already run" : "smi_fusion_run: a segment failed");
        return SMI_ERR_STATE;
    }
    h->ran = true;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    int64_t *c = h->counts;
    const int32_t n = (int32_t)h->names.size(), nF = (int32_t)h->genes.size(), nC = (int32_t)h->cells.size();
    c[SMI_FUS_GENE_FIELDS] = nF;
    int rc = 0;
    Events evt;
    Scratch tmp{kWho};
    auto exclusive_sum = [&](auto *in, auto *out, int m) {
        return run(tmp, [=](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, in, out, m, s); });
    };
    int32_t n_reads = 0, n_mol = 0;
    int64_t n_pairs = 0;
    std::vector<int32_t> mol_n, mol_bc, mol_umi, mol_de, mol_cell, mol_pair, mol_ng;
    std::vector<uint64_t> pair, upair;
    if (n) {
        uint32_t mask_r = 0, mask_g = 0, mask_c = 0, mask_m = 0;
        if ((rc = table_size(h, n, "kept records", &mask_r)) || (rc = table_size(h, nF, "gene fields", &mask_g)) ||
            (rc = table_size(h, nC, "cells", &mask_c)))
            return rc;
        // the pools
        DevBuf<uint8_t> d_name{kWho}, d_bc{kWho}, d_umi{kWho}, d_gene{kWho}, d_cellp{kWho}, d_has{kWho};
        DevBuf<uint64_t> d_name_off{kWho}, d_bc_off{kWho}, d_umi_off{kWho}, d_gene_off{kWho}, d_cell_off{kWho};
        DevBuf<int32_t> d_frec{kWho};
        if ((rc = d_name.put(h->names.bytes, s)) || (rc = d_name_off.put(h->names.off, s)) || (rc = d_bc.put(h->bcs.bytes, s)) ||
            (rc = d_bc_off.put(h->bcs.off, s)) || (rc = d_umi.put(h->umis.bytes, s)) || (rc = d_umi_off.put(h->umis.off, s)) ||
            (rc = d_gene.put(h->genes.bytes, s)) || (rc = d_gene_off.put(h->genes.off, s)) || (rc = d_cellp.put(h->cells.bytes, s)) ||
            (rc = d_cell_off.put(h->cells.off, s)) || (rc = d_has.put(h->has_umi, s)) || (rc = d_frec.put(h->f_rec, s)))
            return rc;
        // counters: probe steps, wraps, reads of several records, distinct genes, multiIG molecules; the overflow flag
        DevBuf<unsigned long long> d_cnt{kWho};
        DevBuf<uint32_t> d_over{kWho};
        if ((rc = d_cnt.alloc(5)) || (rc = d_over.alloc(1))) return rc;
        SMI_HIP(hipMemsetAsync(d_cnt.p, 0, 5 * sizeof(unsigned long long), s));
        SMI_HIP(hipMemsetAsync(d_over.p, 0, sizeof(uint32_t), s));
        auto insert = [&](const Keys &keys, uint32_t nk, uint32_t mask, DevBuf<uint32_t> &tab, int32_t *group) -> int {
            if (int rc2 = tab.alloc((size_t)mask + 1)) return rc2;
            SMI_HIP(hipMemsetAsync(tab.p, 0xff, ((size_t)mask + 1) * 4, s));
            if (!nk) return SMI_OK;
            InsArgs a = {keys, keys, nullptr, nk, mask, tab.p, group, d_cnt.p, d_cnt.p + 1, d_over.p};
            if (int rc2 = evt.begin(s)) return rc2;
            hipLaunchKernelGGL(k_fus_insert<false>, dim3(grid(nk)), dim3(kFusBlock), 0, s, a);
            SMI_HIP(hipGetLastError());
            if (int rc2 = evt.end(s, &ms[0])) return rc2;
            uint32_t over = 0;
            SMI_HIP(hipMemcpy(&over, d_over.p, 4, hipMemcpyDeviceToHost));
            if (over) {  // (cannot happen: every table has at least as many slots as keys)
                set_error("FusionDetector: a K-FUS-INSERT table ran full");
                return SMI_ERR_STATE;
            }
            return SMI_OK;
        };
        // reads
        DevBuf<uint32_t> t_read{kWho}, t_mol{kWho}, t_gene{kWho}, t_cell{kWho};
        DevBuf<int32_t> d_rep{kWho}, d_first{kWho}, d_last{kWho}, d_lumi{kWho}, d_nrec{kWho}, d_flag{kWho}, d_rq{kWho};
        if ((rc = d_rep.alloc(n)) || (rc = d_first.alloc(n)) || (rc = d_last.alloc(n)) || (rc = d_lumi.alloc(n)) || (rc = d_nrec.alloc(n)) ||
            (rc = d_flag.alloc((size_t)n + 1)) || (rc = d_rq.alloc((size_t)n + 1)))
            return rc;
        if ((rc = insert(Keys{d_name.p, d_name_off.p}, (uint32_t)n, mask_r, t_read, d_rep.p))) return rc;
        if ((rc = evt.begin(s))) return rc;
        hipLaunchKernelGGL(k_fus_init, dim3(grid(n)), dim3(kFusBlock), 0, s, d_first.p, d_last.p, d_lumi.p, d_nrec.p, n);
        hipLaunchKernelGGL(k_fus_read, dim3(grid(n)), dim3(kFusBlock), 0, s, d_rep.p, d_has.p, n, d_first.p, d_last.p, d_lumi.p, d_nrec.p);
        hipLaunchKernelGGL(k_fus_flag, dim3(grid((size_t)n + 1)), dim3(kFusBlock), 0, s, d_rep.p, d_first.p, n, d_flag.p);
        SMI_HIP(hipGetLastError());
        if ((rc = exclusive_sum(d_flag.p, d_rq.p, n + 1))) return rc;
        if ((rc = evt.end(s, &ms[1]))) return rc;
        SMI_HIP(hipMemcpy(&n_reads, d_rq.p + n, 4, hipMemcpyDeviceToHost));
        DevBuf<int32_t> d_qfirst{kWho}, d_qlast{kWho}, d_qumi{kWho};
        DevBuf<uint64_t> d_klen{kWho}, d_koff{kWho};
        DevBuf<uint8_t> d_key{kWho};
        if ((rc = d_qfirst.alloc(n_reads)) || (rc = d_qlast.alloc(n_reads)) || (rc = d_qumi.alloc(n_reads)) || (rc = d_klen.alloc((size_t)n_reads + 1)) ||
            (rc = d_koff.alloc((size_t)n_reads + 1)))
            return rc;
        SMI_HIP(hipMemsetAsync(d_klen.p, 0, ((size_t)n_reads + 1) * 8, s));
        {
            ReadArgs a = {d_rep.p, d_flag.p, d_rq.p, d_last.p, d_lumi.p, d_nrec.p, d_bc_off.p, d_umi_off.p, n, d_qfirst.p, d_qlast.p, d_qumi.p, d_klen.p,
                          d_cnt.p + 2};
            if ((rc = evt.begin(s))) return rc;
            hipLaunchKernelGGL(k_fus_read_list, dim3(grid(n)), dim3(kFusBlock), 0, s, a);
            SMI_HIP(hipGetLastError());
            if ((rc = exclusive_sum(d_klen.p, d_koff.p, n_reads + 1))) return rc;
            uint64_t key_bytes = 0;
            SMI_HIP(hipMemcpyAsync(&key_bytes, d_koff.p + n_reads, 8, hipMemcpyDeviceToHost, s));
            SMI_HIP(hipStreamSynchronize(s));
            if ((rc = d_key.alloc(key_bytes))) return rc;
            hipLaunchKernelGGL(k_fus_read_key, dim3(grid(n_reads)), dim3(kFusBlock), 0, s, d_qlast.p, d_qumi.p, n_reads, d_bc.p, d_bc_off.p, d_umi.p,
                               d_umi_off.p, d_koff.p, d_key.p);
            SMI_HIP(hipGetLastError());
            if ((rc = evt.end(s, &ms[1]))) return rc;
        }
        // molecules
        if ((rc = table_size(h, n_reads, "reads", &mask_m))) return rc;
        DevBuf<int32_t> d_mrep{kWho}, d_mfirst{kWho}, d_mlast{kWho}, d_mn{kWho}, d_mflag{kWho}, d_mq{kWho}, d_read_mol{kWho};
        if ((rc = d_mrep.alloc(n_reads)) || (rc = d_mfirst.alloc(n_reads)) || (rc = d_mlast.alloc(n_reads)) || (rc = d_mn.alloc(n_reads)) ||
            (rc = d_mflag.alloc((size_t)n_reads + 1)) || (rc = d_mq.alloc((size_t)n_reads + 1)) || (rc = d_read_mol.alloc(n_reads)))
            return rc;
        if ((rc = insert(Keys{d_key.p, d_koff.p}, (uint32_t)n_reads, mask_m, t_mol, d_mrep.p))) return rc;
        if ((rc = evt.begin(s))) return rc;
        hipLaunchKernelGGL(k_fus_init, dim3(grid(n_reads)), dim3(kFusBlock), 0, s, d_mfirst.p, d_mlast.p, (int32_t *)nullptr, d_mn.p, n_reads);
        hipLaunchKernelGGL(k_fus_mol, dim3(grid(n_reads)), dim3(kFusBlock), 0, s, d_mrep.p, n_reads, d_mfirst.p, d_mlast.p, d_mn.p);
        hipLaunchKernelGGL(k_fus_flag, dim3(grid((size_t)n_reads + 1)), dim3(kFusBlock), 0, s, d_mrep.p, d_mfirst.p, n_reads, d_mflag.p);
        SMI_HIP(hipGetLastError());
        if ((rc = exclusive_sum(d_mflag.p, d_mq.p, n_reads + 1))) return rc;
        if ((rc = evt.end(s, &ms[2]))) return rc;
        SMI_HIP(hipMemcpy(&n_mol, d_mq.p + n_reads, 4, hipMemcpyDeviceToHost));
        DevBuf<int32_t> d_mol_n{kWho}, d_mol_bc{kWho}, d_mol_umi{kWho}, d_mol_de{kWho}, d_mol_ng{kWho}, d_mol_gs{kWho}, d_mol_cell{kWho}, d_mol_pair{kWho};
        if ((rc = d_mol_n.alloc(n_mol)) || (rc = d_mol_bc.alloc(n_mol)) || (rc = d_mol_umi.alloc(n_mol)) || (rc = d_mol_de.alloc(n_mol)) ||
            (rc = d_mol_ng.alloc(n_mol)) || (rc = d_mol_gs.alloc(n_mol)) || (rc = d_mol_cell.alloc(n_mol)) || (rc = d_mol_pair.alloc(n_mol)))
            return rc;
        {
            MolArgs a = {d_mrep.p, d_mflag.p, d_mq.p, d_mfirst.p, d_mlast.p, d_mn.p, d_qfirst.p, d_qlast.p, d_qumi.p, n_reads, d_read_mol.p,
                         d_mol_n.p, d_mol_bc.p, d_mol_umi.p, d_mol_de.p};
            if ((rc = evt.begin(s))) return rc;
            hipLaunchKernelGGL(k_fus_mol_list, dim3(grid(n_reads)), dim3(kFusBlock), 0, s, a);
            SMI_HIP(hipGetLastError());
            if ((rc = evt.end(s, &ms[2]))) return rc;
        }
        // the cell list: its table, then contains(molecule.getBarcode()) per molecule
        DevBuf<int32_t> d_cgroup{kWho};
        if ((rc = d_cgroup.alloc(nC))) return rc;
        if ((rc = insert(Keys{d_cellp.p, d_cell_off.p}, (uint32_t)nC, mask_c, t_cell, d_cgroup.p))) return rc;
        {
            InsArgs a = {Keys{d_cellp.p, d_cell_off.p}, Keys{d_bc.p, d_bc_off.p}, d_mol_bc.p, (uint32_t)n_mol, mask_c, t_cell.p, d_mol_cell.p, d_cnt.p,
                         d_cnt.p + 1, d_over.p};
            if ((rc = evt.begin(s))) return rc;
            hipLaunchKernelGGL(k_fus_insert<true>, dim3(grid(n_mol)), dim3(kFusBlock), 0, s, a);
            SMI_HIP(hipGetLastError());
            if ((rc = evt.end(s, &ms[0]))) return rc;
        }
        // genes
        DevBuf<int32_t> d_grep{kWho}, d_gfirst{kWho};
        DevBuf<uint64_t> d_code{kWho}, d_sorted{kWho}, d_ucode{kWho}, d_pair{kWho}, d_psorted{kWho}, d_upair{kWho};
        DevBuf<uint32_t> d_rl{kWho};
        DevBuf<int64_t> d_nrun{kWho};
        if ((rc = d_grep.alloc(nF)) || (rc = d_gfirst.alloc(nF)) || (rc = d_code.alloc(nF)) || (rc = d_sorted.alloc(nF)) || (rc = d_ucode.alloc(nF)) ||
            (rc = d_rl.alloc(std::max(nF, n_mol))) || (rc = d_nrun.alloc(2)) || (rc = d_pair.alloc(n_mol)) || (rc = d_psorted.alloc(n_mol)) ||
            (rc = d_upair.alloc(n_mol)))
            return rc;
        SMI_HIP(hipMemsetAsync(d_nrun.p, 0, 16, s));
        if ((rc = insert(Keys{d_gene.p, d_gene_off.p}, (uint32_t)nF, mask_g, t_gene, d_grep.p))) return rc;
        if ((rc = evt.begin(s))) return rc;
        hipLaunchKernelGGL(k_fus_init, dim3(grid(n_mol)), dim3(kFusBlock), 0, s, (int32_t *)nullptr, (int32_t *)nullptr, d_mol_gs.p, d_mol_ng.p, n_mol);
        if (nF) {
            hipLaunchKernelGGL(k_fus_init, dim3(grid(nF)), dim3(kFusBlock), 0, s, d_gfirst.p, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, nF);
            hipLaunchKernelGGL(k_fus_gene_first, dim3(grid(nF)), dim3(kFusBlock), 0, s, d_grep.p, nF, d_gfirst.p);
            CodeArgs a = {d_grep.p, d_gfirst.p, d_frec.p, d_rep.p, d_first.p, d_rq.p, d_read_mol.p, nF, d_code.p, d_cnt.p + 3};
            hipLaunchKernelGGL(k_fus_codes, dim3(grid(nF)), dim3(kFusBlock), 0, s, a);
            SMI_HIP(hipGetLastError());
            if ((rc = sort_rle(s, d_code.p, d_sorted.p, d_ucode.p, d_rl.p, d_nrun.p, nF, 64).run(tmp))) return rc;
            hipLaunchKernelGGL(k_fus_gene_count, dim3(grid(nF)), dim3(kFusBlock), 0, s, d_ucode.p, d_nrun.p, d_mol_ng.p, d_mol_gs.p);
        }
        {
            SelArgs a = {d_mol_ng.p, d_mol_gs.p, d_mol_umi.p, d_mol_cell.p, d_ucode.p, Keys{d_gene.p, d_gene_off.p}, n_mol, d_pair.p, d_cnt.p + 4};
            hipLaunchKernelGGL(k_fus_select, dim3(grid(n_mol)), dim3(kFusBlock), 0, s, a);
            SMI_HIP(hipGetLastError());
            if ((rc = sort_rle(s, d_pair.p, d_psorted.p, d_upair.p, d_rl.p, d_nrun.p + 1, n_mol, 64).run(tmp))) return rc;
            hipLaunchKernelGGL(k_fus_pair_id, dim3(grid(n_mol)), dim3(kFusBlock), 0, s, d_pair.p, n_mol, d_upair.p, d_nrun.p + 1, d_mol_pair.p);
            SMI_HIP(hipGetLastError());
        }
        if ((rc = evt.end(s, &ms[3]))) return rc;
        // back to the host
        unsigned long long cnt[5];
        SMI_HIP(hipMemcpy(cnt, d_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(&n_pairs, d_nrun.p + 1, 8, hipMemcpyDeviceToHost));
        c[SMI_FUS_PROBE_STEPS] = (int64_t)cnt[0];
        c[SMI_FUS_WRAPS] = (int64_t)cnt[1];
        c[SMI_FUS_READS_MULTI] = (int64_t)cnt[2];
        c[SMI_FUS_GENES] = (int64_t)cnt[3];
        c[SMI_FUS_MULTI_IG] = (int64_t)cnt[4];
        auto get = [&](std::vector<int32_t> &v, const DevBuf<int32_t> &d) -> int {
            v.resize(n_mol);
            SMI_HIP(hipMemcpy(v.data(), d.p, (size_t)n_mol * 4, hipMemcpyDeviceToHost));
            return SMI_OK;
        };
        if ((rc = get(mol_n, d_mol_n)) || (rc = get(mol_bc, d_mol_bc)) || (rc = get(mol_umi, d_mol_umi)) || (rc = get(mol_de, d_mol_de)) ||
            (rc = get(mol_cell, d_mol_cell)) || (rc = get(mol_pair, d_mol_pair)) || (rc = get(mol_ng, d_mol_ng)))
            return rc;
        pair.resize(n_mol);
        upair.resize(n_pairs);
        SMI_HIP(hipMemcpy(pair.data(), d_pair.p, (size_t)n_mol * 8, hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(upair.data(), d_upair.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
        if (!upair.empty() && upair.back() == kNoPair) upair.pop_back();  // the molecules that are not counted
    }
    c[SMI_FUS_READS] = n_reads;
    c[SMI_FUS_MOLECULES] = n_mol;
    c[SMI_FUS_MOLECULE_READS] = n_reads;  // every read is in one molecule (MoleculeDataset L92)
    // the label of every pair: set.toString() through the three replace calls (FusionDetector.java L82-85); rows = distinct labels, sorted
    std::vector<std::string> pair_label(upair.size()), rows;
    for (size_t k = 0; k < upair.size(); k++) {
        std::string key = "[" + std::string(h->genes.at(upair[k] >> 32)) + ", " + std::string(h->genes.at((uint32_t)upair[k])) + "]";
        key = jreplace(key, ", ", "|");
        key = jreplace(key, "[", "");
        key = jreplace(key, "]", "");
        pair_label[k] = key;
    }
    rows = pair_label;
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    std::vector<int32_t> pair_row(upair.size());
    for (size_t k = 0; k < upair.size(); k++) pair_row[k] = (int32_t)(std::lower_bound(rows.begin(), rows.end(), pair_label[k]) - rows.begin());
    // K-MTX: one code per counted molecule (a molecule is one UMI of its cell: Matrix.addMolecule L62-105)
    std::vector<int32_t> counted;
    std::vector<uint64_t> codes;
    for (int32_t j = 0; j < n_mol; j++)
        if (mol_pair[j] >= 0) {
            counted.push_back(j);
            codes.push_back((uint64_t)(uint32_t)pair_row[mol_pair[j]] << 32 | (uint32_t)mol_cell[j]);
        }
    c[SMI_FUS_COUNTED] = (int64_t)counted.size();
    c[SMI_FUS_ROWS] = (int64_t)rows.size();
    std::vector<std::string> labels(rows.size());
    for (size_t r = 0; r < rows.size(); r++) labels[r] = rows[r] + "\t" + rows[r] + "\tna";
    std::string &mat = h->out[SMI_FUS_OUT_MATRIX];
    mat = "geneId\ttranscriptId\tnbExons";
    for (int32_t k = 0; k < nC; k++) {
        mat += '\t';
        mat.append(h->cells.at(k));
    }
    mat += '\n';
    std::vector<int64_t> row_total;
    if ((rc = mtx::matrix(s, "FusionDetector", nC, h->cfg.budget_bytes, codes, labels, mat, row_total, &ms[4], &ms[5], &c[SMI_FUS_RENDER_BLOCKS])))
        return rc;
    std::string &met = h->out[SMI_FUS_OUT_METRICS];
    met = "geneId\ttranscriptId\tnbExons\tnbUmis\n";
    for (size_t r = 0; r < rows.size(); r++) met += labels[r] + "\t" + std::to_string(row_total[r]) + "\n";
    // molinfos in (cell, UMI) byte order; the cells are numbered in byte order
    std::sort(counted.begin(), counted.end(), [&](int32_t x, int32_t y) {
        return mol_cell[x] != mol_cell[y] ? mol_cell[x] < mol_cell[y] : h->umis.at(mol_umi[x]) < h->umis.at(mol_umi[y]);
    });
    std::string &mol = h->out[SMI_FUS_OUT_MOLINFOS];
    mol = "cellBC\tUMI\tnbReads\tnbSupportingReads\tmappingPctId\tsnpPhredScore\tgeneId\ttranscriptId\n";
    for (int32_t j : counted) {
        const int32_t rn = h->rn[mol_bc[j]];  // Molecule.rn: the first read's rn, which is its last record's
        const int32_t nreads = rn > 1 ? rn : mol_n[j];
        const float pct = 1.0f - h->de[mol_de[j]];
        const std::string &key = pair_label[mol_pair[j]];
        mol.append(h->bcs.at(mol_bc[j]));
        mol += '\t';
        mol.append(h->umis.at(mol_umi[j]));
        mol += "\t" + std::to_string(nreads) + "\t0\t" + lr::java_float(pct) + "\t\t" + key + "\t" + key + "\n";
    }
    h->k_ng = std::move(mol_ng);
    h->k_pair = std::move(pair);
    if (stage_ms) std::memcpy(stage_ms, ms, sizeof(ms));
    return SMI_OK;
}

// the reference's loops as it runs them: LongreadParser L61-79 (reads by name), MoleculeDataset L69-84 (molecules by key, the reads in the
// order of their first record), FusionDetector.java L76-92 (the selection and the set's order), one thread, ordinary hash maps
extern "C" int smi_fusion_host_loop(const smi_fusion *h, double *seconds, int64_t *mismatches) {
    if (!h || !seconds || !mismatches) {
        set_error("smi_fusion_host_loop: null argument");
        return SMI_ERR_INVALID;
    }
    if (!h->ran) {
        set_error("smi_fusion_host_loop: smi_fusion_run comes first");
        return SMI_ERR_STATE;
    }
    struct Read {
        std::unordered_set<std::string_view> genes;
        int32_t last = -1, umi = -1;
    };
    struct Mol {
        std::unordered_set<std::string_view> genes;
        int32_t bc = -1, umi = -1;
    };
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t n = (int32_t)h->names.size();
    std::unordered_map<std::string_view, int32_t> read_of;
    std::vector<Read> reads;
    for (int32_t r = 0; r < n; r++) {
        auto it = read_of.emplace(h->names.at(r), (int32_t)reads.size());
        if (it.second) reads.emplace_back();
        Read &rd = reads[it.first->second];
        for (int32_t f = h->f_start[r]; f < h->f_start[r + 1]; f++) rd.genes.insert(h->genes.at(f));
        rd.last = r;
        if (h->has_umi[r]) rd.umi = r;
    }
    std::unordered_map<std::string, int32_t> mol_of;
    std::vector<Mol> mols;
    std::string key;
    for (const Read &rd : reads) {
        key.assign(h->bcs.at(rd.last));
        key += ':';
        if (rd.umi >= 0) key.append(h->umis.at(rd.umi));
        key += rd.umi >= 0 ? '\1' : '\0';
        auto it = mol_of.emplace(key, (int32_t)mols.size());
        if (it.second) {
            mols.emplace_back();
            mols.back().bc = rd.last;
            mols.back().umi = rd.umi;
        }
        Mol &m = mols[it.first->second];
        for (auto g : rd.genes) m.genes.insert(g);
    }
    std::unordered_set<std::string_view> listed;
    for (size_t k = 0; k < h->cells.size(); k++) listed.insert(h->cells.at(k));
    std::vector<std::string_view> first(mols.size()), second(mols.size());
    std::vector<uint8_t> sel(mols.size(), 0);
    for (size_t j = 0; j < mols.size(); j++) {
        const Mol &m = mols[j];
        if (!(listed.count(h->bcs.at(m.bc)) && m.umi >= 0 && m.genes.size() == 2)) continue;
        auto it = m.genes.begin();
        std::string_view a = *it++, b = *it;
        const uint32_t ba = java_bucket_host(a), bb = java_bucket_host(b);
        if (bb < ba || (ba == bb && b < a)) std::swap(a, b);
        first[j] = a;
        second[j] = b;
        sel[j] = 1;
    }
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *mismatches = mols.size() > h->k_ng.size() ? (int64_t)(mols.size() - h->k_ng.size()) : (int64_t)(h->k_ng.size() - mols.size());
    for (size_t j = 0; j < std::min(mols.size(), h->k_ng.size()); j++) {
        const bool dsel = h->k_pair[j] != kNoPair;
        bool same = (int64_t)mols[j].genes.size() == h->k_ng[j] && dsel == (bool)sel[j];
        if (same && dsel) same = h->genes.at(h->k_pair[j] >> 32) == first[j] && h->genes.at((uint32_t)h->k_pair[j]) == second[j];
        *mismatches += !same;
    }
    return SMI_OK;
}
