// smi_clipexport.hip -- `ExportClippedReads` (org/ipmc/sicelore/programs/ExportClippedReads.java:L50-104, the first program of the reference
// README's step 6): the records of a BAM with a long soft or hard clip at either end, written once per key as a FASTQ record whose name is
// the key: <read name up to its first '_'>_<GE>_<BC>_<U8>, sequence and qualities from US / QS.  The rules are DESIGN.md section 8k's;
// tests/fusionprepmodel.py implements the same ones.
//
// The BAM comes in segments (smi_clipexport_segment); per segment:
//   K-CLIP-FLAG    one lane per record: the first and the last CIGAR word (L78-85), the five attributes by one walk over the record's
//                  attributes (lr::aux_size; a repeated tag keeps its last value), the name up to its first '_' (L68, L76);
//                  -> clipped or not, the length of the key, and the records the reference's loop dies on (atomicMin of the record index)
//   K-CLIP-KEY     hipcub exclusive scan of the key lengths, then the keys of the clipped records into the segment's byte pool
//   K-CLIP-INSERT  the HashSet of L58 / L87 / L94 as an open-addressing table over the key bytes, walked by probe() of smi_device.h as
//                  K-FUS-INSERT and K-DD-INSERT walk theirs: 64-bit FNV-1a, a key claims an empty slot by CAS or joins the slot's key when
//                  length and bytes are equal, else probes on, wrapping at the end.  The table and the pool of the keys written so far stay on the device across
//                  segments: an entry below `resident` is a key of an earlier segment (the record loses), any other entry is a record of
//                  this segment, and among the records of one key the smallest record index wins (atomicMin).  Which record of a group
//                  holds the slot is a race; what is written is not.
//   K-CLIP-PICK    winners, their FASTQ sizes, the group representatives (the new resident keys); three exclusive scans
//   K-CLIP-COMMIT  the new keys behind the resident pool, the table's entries of this segment renumbered to resident key numbers
//   K-CLIP-WRITE   one wavefront per winner: key, US and QS copied byte-wise up to the destination's 4-byte boundary, then as whole dwords,
//                  then the tail (as K-DD-WRITE copies); lane 0 writes '@', the '+' line and the line ends
#include <chrono>
#include <climits>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_set>
#include <vector>

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"  // put_field: K-EDIT's, not used here
#include "smi_auxedit.h"
#pragma clang diagnostic pop
#include "smi_handle.h"
#include "smi_internal.h"

namespace smi {
namespace {

constexpr int kClipBlock = 256;
constexpr int kClipWaves = 4;  // waves per block of K-CLIP-WRITE
constexpr unsigned long long kNoRecord = ~0ull;
constexpr int kTags = 5;  // GENETAG, CELLTAG, UMITAG, USTAG, QSTAG

// ClipRec.flags
enum : uint32_t {
    CLIP_CLIPPED = 1,      // L82-85
    CLIP_BAD_READ = 2,     // US or QS is no string: fatal only where the record is written (L91-92)
    CLIP_KIND_SHIFT = 8,   // bits 8 ..: why the reference's loop dies on this record (0: it does not)
};
enum : uint32_t { STOP_TAG = 1, STOP_NAME = 2, STOP_NO_CIGAR = 3, STOP_EQ_CLIP = 4 };

struct ClipRec {
    uint64_t val[kTags];  // offset of the value in the BAM buffer (a missing attribute: the bytes "null" behind the buffer)
    uint32_t len[kTags];
    uint32_t tmp0_len;  // the name up to its first '_'
    uint32_t klen;      // bytes of the key; 0: not clipped
    uint32_t flags;
};

struct FlagArgs {
    const uint8_t *bam;
    const smi_bam_record *recs;
    uint32_t n;
    uint32_t key[kTags];
    int64_t min_clip;
    uint64_t null_off;
    ClipRec *out;
    uint64_t *klen;             // [n + 1], the last one 0
    unsigned long long *words;  // W_*
};
enum { W_ERR = 0, W_CLIPPED, W_WINNERS, W_STEPS, W_WRAPS, W_BAD, W_COUNT };

__global__ __launch_bounds__(kClipBlock) void k_clip_flag(FlagArgs a) {
    const uint32_t i = blockIdx.x * kClipBlock + threadIdx.x;
    bool clipped = false;
    if (i == a.n) a.klen[i] = 0;  // the scan's total
    if (i < a.n) {
        const smi_bam_record r = a.recs[i];
        ClipRec o;
        uint8_t st[kTags];  // 0 missing, 1 Z, 2 any other type
#pragma unroll
        for (int t = 0; t < kTags; t++) {
            o.val[t] = a.null_off;
            o.len[t] = 4;
            st[t] = 0;
        }
        const uint64_t end = r.aux_off + r.aux_len;
        bool bad_aux = false;
        for (uint64_t p = r.aux_off; p < end;) {
            size_t size;
            if (lr::aux_size(a.bam + p, a.bam + end, &size)) {
                bad_aux = true;
                break;
            }
            const uint64_t q = p + size;
            const uint32_t key = (uint32_t)a.bam[p + 1] << 8 | a.bam[p];
            const bool z = a.bam[p + 2] == 'Z';
#pragma unroll
            for (int t = 0; t < kTags; t++)
                if (key == a.key[t]) {
                    st[t] = z ? 1 : 2;
                    o.val[t] = z ? p + 3 : a.null_off;
                    o.len[t] = z ? (uint32_t)(q - p - 4) : 4;
                }
            p = q;
        }
        if (bad_aux) atomicOr(a.words + W_BAD, 1ull);
        // readName.split("_")[0]
        const uint8_t *s = a.bam + r.name_off;
        const uint32_t len = r.l_read_name ? r.l_read_name - 1u : 0u;
        uint32_t us = len;
        bool other = false;
        for (uint32_t k = 0; k < len; k++) {
            if (s[k] == '_') {
                if (us == len) us = k;
            } else
                other = true;
        }
        o.tmp0_len = us;
        uint32_t stop = 0;
        if (st[0] == 2 || st[1] == 2 || st[2] == 2) stop = STOP_TAG;  // (String) getAttribute, L72-74
        else if (len && !other) stop = STOP_NAME;                     // tmp[0] of an empty array, L76
        else if (r.n_cigar == 0) stop = STOP_NO_CIGAR;                // cigartype[1] of "*", L82
        else {
            const uint32_t c0 = ld_u32(a.bam + r.cigar_off), c1 = ld_u32(a.bam + r.cigar_off + 4ull * (r.n_cigar - 1u));
            const uint32_t op0 = c0 & 15, op1 = c1 & 15;
            // L84: the last piece of split("[A-Z]") is "<n>=<m>" when '=' stands in front of the last operation
            if ((op1 == 4 || op1 == 5) && r.n_cigar >= 2 && (ld_u32(a.bam + r.cigar_off + 4ull * (r.n_cigar - 2u)) & 15) == 7) stop = STOP_EQ_CLIP;
            else
                clipped = ((op0 == 4 || op0 == 5) && (int64_t)(c0 >> 4) > a.min_clip) || ((op1 == 4 || op1 == 5) && (int64_t)(c1 >> 4) > a.min_clip);
        }
        o.klen = clipped ? o.tmp0_len + o.len[0] + o.len[1] + o.len[2] + 3u : 0u;
        o.flags = (clipped ? CLIP_CLIPPED : 0u) | (st[3] == 2 || st[4] == 2 ? CLIP_BAD_READ : 0u) | stop << CLIP_KIND_SHIFT;
        if (stop) atomicMin(a.words + W_ERR, (unsigned long long)i);
        a.out[i] = o;
        a.klen[i] = o.klen;
    }
    const unsigned long long m = __ballot(clipped);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.words + W_CLIPPED, (unsigned long long)__popcll(m));
}

// K-CLIP-KEY: tmp[0] + "_" + geneId + "_" + barcode + "_" + umi (L76) of every clipped record
__global__ __launch_bounds__(kClipBlock) void k_clip_key(const uint8_t *__restrict__ bam, const smi_bam_record *__restrict__ recs,
                                                         const ClipRec *__restrict__ cr, const uint64_t *__restrict__ koff, uint32_t n,
                                                         uint8_t *__restrict__ pool) {
    const uint32_t i = blockIdx.x * kClipBlock + threadIdx.x;
    if (i >= n) return;
    const ClipRec c = cr[i];
    if (!c.klen) return;
    uint8_t *dst = pool + koff[i];
    const uint8_t *s = bam + recs[i].name_off;
    uint32_t k = 0;
    for (uint32_t b = 0; b < c.tmp0_len; b++) dst[k++] = s[b];
#pragma unroll
    for (int t = 0; t < 3; t++) {
        dst[k++] = '_';
        const uint8_t *v = bam + c.val[t];
        for (uint32_t b = 0; b < c.len[t]; b++) dst[k++] = v[b];
    }
}

// K-CLIP-INSERT.  Table entries: e < resident: key e of the resident pool; else candidate e - resident of this call.  Candidate i is
// spool[soff[i] .. soff[i + 1]); an empty one takes no part.  group[i] = the entry that holds the candidate's key (kEmpty: no candidate,
// or the table ran full: *overflow set).  first[c] (may be null) = the smallest candidate whose key candidate c's entry holds.
struct InsArgs {
    const uint8_t *rpool;
    const uint64_t *roff;
    const uint8_t *spool;
    const uint64_t *soff;
    uint32_t resident, n, mask;
    uint32_t *tab, *group, *first;
    unsigned long long *words;
};

__global__ __launch_bounds__(kClipBlock) void k_clip_insert(InsArgs a) {
    const uint32_t i = blockIdx.x * kClipBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t o = a.soff[i];
    const uint32_t len = (uint32_t)(a.soff[i + 1] - o);
    uint32_t res = kEmpty;
    if (len) {
        const Bytes mine = {a.spool + o, len};
        const uint64_t h = fnv1a(mine.p, len);
        const uint8_t *rpool = a.rpool, *spool = a.spool;
        const uint64_t *roff = a.roff, *soff = a.soff;
        const uint32_t resident = a.resident;
        const Probed p = probe<true>(a.tab, a.mask, (uint32_t)(h ^ (h >> 32)) & a.mask, resident + i, mine, [=](uint32_t e) {
            const bool old = e < resident;
            const uint64_t *off = old ? roff + e : soff + (e - resident);
            return Bytes{(old ? rpool : spool) + off[0], (uint32_t)(off[1] - off[0])};
        });
        res = p.entry;
        if (res == kEmpty) atomicOr(a.words + W_BAD, 2ull);
        else if (a.first && res >= a.resident) atomicMin(&a.first[res - a.resident], i);
        if (p.steps) atomicAdd(a.words + W_STEPS, (unsigned long long)p.steps);
        if (p.wraps) atomicAdd(a.words + W_WRAPS, (unsigned long long)p.wraps);
    }
    if (a.group) a.group[i] = res;
}

// K-CLIP-PICK: record i is written when its key is new in this segment and i is the smallest record of the key (L87); the record whose
// entry holds the key hands it to the resident pool
struct PickArgs {
    const ClipRec *cr;
    const uint32_t *group, *first;
    uint32_t resident, n;
    uint64_t *osize, *rflag, *rsize;  // [n + 1] each, the last one 0
    uint32_t *wlist;
    uint8_t *decision;  // bit 0 clipped, bit 1 written
    unsigned long long *words;
};

__global__ __launch_bounds__(kClipBlock) void k_clip_pick(PickArgs a) {
    const uint32_t i = blockIdx.x * kClipBlock + threadIdx.x;
    if (i > a.n) return;
    uint64_t os = 0, rf = 0, rs = 0;
    if (i < a.n) {
        const ClipRec c = a.cr[i];
        bool win = false;
        if (c.klen) {
            const uint32_t g = a.group[i];
            win = g != kEmpty && g >= a.resident && a.first[g - a.resident] == i;
            if (g == a.resident + i) {
                rf = 1;
                rs = c.klen;
            }
        }
        if (win) {
            os = (uint64_t)c.klen + c.len[3] + c.len[4] + 6;  // '@' key \n US \n + \n QS \n
            if (c.flags & CLIP_BAD_READ) atomicMin(a.words + W_ERR, (unsigned long long)i);
            a.wlist[atomicAdd(a.words + W_WINNERS, 1ull)] = i;
        }
        a.decision[i] = (uint8_t)((c.flags & CLIP_CLIPPED) | (win ? 2u : 0u));
    }
    a.osize[i] = os;
    a.rflag[i] = rf;
    a.rsize[i] = rs;
}

// K-CLIP-COMMIT 1: the keys of the representatives behind the resident pool, numbered resident + rnew[i]
__global__ __launch_bounds__(kClipBlock) void k_clip_commit(const uint64_t *__restrict__ rflag, const uint64_t *__restrict__ rnew,
                                                            const uint64_t *__restrict__ rkoff, const uint8_t *__restrict__ spool,
                                                            const uint64_t *__restrict__ soff, uint32_t n, uint32_t resident, uint64_t resident_bytes,
                                                            uint8_t *__restrict__ rpool, uint64_t *__restrict__ roff) {
    const uint32_t i = blockIdx.x * kClipBlock + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        roff[resident + rnew[n]] = resident_bytes + rkoff[n];  // the end of the last key
        return;
    }
    if (!rflag[i]) return;
    const uint64_t to = resident_bytes + rkoff[i], from = soff[i];
    const uint32_t len = (uint32_t)(soff[i + 1] - from);
    roff[resident + rnew[i]] = to;
    for (uint32_t k = 0; k < len; k++) rpool[to + k] = spool[from + k];
}

// K-CLIP-COMMIT 2: the entries of this segment's candidates become resident key numbers
__global__ __launch_bounds__(kClipBlock) void k_clip_remap(uint32_t *__restrict__ tab, uint32_t slots, uint32_t resident, const uint64_t *__restrict__ rnew) {
    const uint32_t s = blockIdx.x * kClipBlock + threadIdx.x;
    if (s >= slots) return;
    const uint32_t v = tab[s];
    if (v != kEmpty && v >= resident) tab[s] = resident + (uint32_t)rnew[v - resident];
}

// K-CLIP-WRITE: "@" + readName + "\n" + US + "\n+\n" + QS + "\n" (L93)
__global__ __launch_bounds__(64 * kClipWaves) void k_clip_write(const uint8_t *__restrict__ bam, const ClipRec *__restrict__ cr,
                                                                const uint32_t *__restrict__ wlist, uint32_t n_win, const uint8_t *__restrict__ spool,
                                                                const uint64_t *__restrict__ soff, const uint64_t *__restrict__ ooff,
                                                                uint8_t *__restrict__ out, uint64_t out_cap) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x * kClipWaves + (threadIdx.x >> 6);
    if (w >= n_win) return;
    const uint32_t i = wlist[w];
    const ClipRec c = cr[i];
    const uint64_t o = ooff[i], total = (uint64_t)c.klen + c.len[3] + c.len[4] + 6;
    if (o + total > out_cap) return;  // (cannot happen: out holds the scan's total)
    uint8_t *dst = out + o, *seq = dst + 1 + c.klen + 1, *qual = seq + c.len[3] + 3;
    if (lane == 0) {
        dst[0] = '@';
        seq[-1] = '\n';
        seq[c.len[3]] = '\n';
        seq[c.len[3] + 1] = '+';
        seq[c.len[3] + 2] = '\n';
        qual[c.len[4]] = '\n';
    }
    wave_copy(dst + 1, spool + soff[i], c.klen, lane);
    wave_copy(seq, bam + c.val[3], c.len[3], lane);
    wave_copy(qual, bam + c.val[4], c.len[4], lane);
}

inline unsigned grid(size_t n) { return (unsigned)std::max<size_t>(1, (n + kClipBlock - 1) / kClipBlock); }

// a device array of at least `want` elements whose first `used` elements are kept
template <class T>
int grow_keep(T **p, size_t &cap, size_t used, size_t want, hipStream_t s) {
    if (want <= cap && *p) return SMI_OK;
    const size_t n = std::max<size_t>(want + want / 2, 1024);
    T *q = nullptr;
    SMI_HIP(hipMalloc((void **)&q, n * sizeof(T)));
    if (*p && used) {
        hipError_t e = hipMemcpyAsync(q, *p, used * sizeof(T), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(q);
            return hip_fail(e, "hipMemcpyAsync");
        }
    }
    if (*p) SMI_HIP(hipFree(*p));
    *p = q;
    cap = n;
    return SMI_OK;
}

const char *const kStopText[5] = {
    "its USTAG or QSTAG attribute is no string and the record would be written (ClassCastException in ExportClippedReads.java:L91-92)",
    "its GENETAG, CELLTAG or UMITAG attribute is no string (ClassCastException in ExportClippedReads.java:L72-74)",
    "its name holds nothing but '_' (ArrayIndexOutOfBoundsException in ExportClippedReads.java:L76)",
    "it has no CIGAR (ArrayIndexOutOfBoundsException in ExportClippedReads.java:L82)",
    "its last clip stands directly behind an '=' operation (NumberFormatException in ExportClippedReads.java:L84)",
};

}  // namespace
}  // namespace smi

using namespace smi;

struct smi_clipexport {
    smi_ctx *ctx = nullptr;
    smi_clipexport_config cfg = {};
    // resident across segments: the keys written so far and the table over them
    uint8_t *d_rpool = nullptr;
    uint64_t *d_roff = nullptr;
    size_t rpool_cap = 0, roff_cap = 0;
    uint32_t resident = 0;
    uint64_t resident_bytes = 0;
    uint32_t *d_tab = nullptr;
    uint64_t slots = 0;
    // one segment (grow-only)
    uint8_t *d_bam = nullptr, *d_spool = nullptr, *d_decision = nullptr, *d_out = nullptr;
    smi_bam_record *d_recs = nullptr;
    ClipRec *d_cr = nullptr;
    uint64_t *d_scan = nullptr;  // 8 arrays of n + 1: klen, koff, osize, ooff, rflag, rnew, rsize, rkoff
    uint32_t *d_group = nullptr, *d_first = nullptr, *d_wlist = nullptr;
    size_t bam_cap = 0, spool_cap = 0, decision_cap = 0, out_cap = 0, recs_cap = 0, cr_cap = 0, scan_cap = 0, group_cap = 0, first_cap = 0, wlist_cap = 0;
    Scratch cub{"ExportClippedReads"};  // hipcub's, kept across segments
    unsigned long long *d_words = nullptr;
    hipEvent_t ev[2] = {};
    // the segment the last call sized and did not write
    const uint8_t *last_bam = nullptr;
    const smi_bam_record *last_recs = nullptr;
    size_t last_n_bam = 0;
    int32_t last_n = -1;
    uint64_t last_total = 0;
    uint32_t last_winners = 0;
    int64_t counts[SMI_CLIP_N_COUNT] = {};
    float ms[SMI_CLIP_N_STAGE] = {};
    std::string error_read;
    int64_t error_record = -1;
    bool failed = false;
    bool dirty = false;  // the table holds entries of a segment that was not committed (a call failed between insert and commit)
    // keep_records: what the reference's loop reads of every record, and the device's decision, for smi_clipexport_host_loop
    struct Kept {
        std::string name, tag[3];
        uint8_t has[3];
        std::vector<uint32_t> cigar;
        uint8_t decision;
    };
    std::vector<Kept> kept;
};

namespace {

void clip_release(smi_clipexport *h) {
    void *bufs[] = {h->d_rpool, h->d_roff, h->d_tab, h->d_bam, h->d_spool, h->d_decision, h->d_out, h->d_recs, h->d_cr, h->d_scan, h->d_group, h->d_first,
                    h->d_wlist, h->d_words};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
}

int clip_scan(smi_clipexport *h, hipStream_t s, const uint64_t *in, uint64_t *out, size_t n) {
    return run(h->cub, [=](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, in, out, n, s); });
}

// a table of at least 2 x keys slots, a power of two; when the present one is smaller, a new one is filled from the resident pool
int clip_table(smi_clipexport *h, hipStream_t s, uint64_t keys) {
    uint64_t want = h->slots ? h->slots : h->cfg.table_log2 ? 1ull << h->cfg.table_log2 : 1024;
    while (want < 2 * keys) want <<= 1;
    if (want == h->slots && h->d_tab) return SMI_OK;
    if (want > (1ull << 31)) {
        set_error("ExportClippedReads: more than 2^30 distinct keys");
        return SMI_ERR_INVALID;
    }
    if (h->d_tab) SMI_HIP(hipFree(h->d_tab));
    h->d_tab = nullptr;
    SMI_HIP(hipMalloc((void **)&h->d_tab, want * sizeof(uint32_t)));
    SMI_HIP(hipMemsetAsync(h->d_tab, 0xff, want * sizeof(uint32_t), s));
    if (h->slots) h->counts[SMI_CLIP_TABLE_GROWS]++;
    h->slots = want;
    h->counts[SMI_CLIP_TABLE_SLOTS] = (int64_t)want;
    if (h->resident) {
        InsArgs a = {h->d_rpool, h->d_roff, h->d_rpool, h->d_roff, 0u, h->resident, (uint32_t)(want - 1), h->d_tab, nullptr, nullptr, h->d_words};
        hipLaunchKernelGGL(k_clip_insert, dim3(grid(h->resident)), dim3(kClipBlock), 0, s, a);
        SMI_HIP(hipGetLastError());
    }
    return SMI_OK;
}

}  // namespace

extern "C" int smi_clipexport_default_config(smi_clipexport_config *cfg) {
    if (!cfg) {
        set_error("smi_clipexport_default_config: null argument");
        return SMI_ERR_INVALID;
    }
    *cfg = {};
    cfg->min_clip = 150;
    std::memcpy(cfg->cell_tag, "BC", 3);
    std::memcpy(cfg->umi_tag, "U8", 3);
    std::memcpy(cfg->gene_tag, "GE", 3);
    std::memcpy(cfg->us_tag, "US", 3);
    std::memcpy(cfg->qs_tag, "QS", 3);
    return SMI_OK;
}

extern "C" int smi_clipexport_create(smi_ctx *ctx, const smi_clipexport_config *cfg, smi_clipexport **out) {
    if (!ctx || !cfg || !out) {
        set_error("smi_clipexport_create: null argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    const char *tags[kTags] = {cfg->gene_tag, cfg->cell_tag, cfg->umi_tag, cfg->us_tag, cfg->qs_tag};
    const char *names[kTags] = {"GENETAG", "CELLTAG", "UMITAG", "USTAG", "QSTAG"};
    for (int k = 0; k < kTags; k++)
        if (!valid_tag(tags[k])) {
            set_error(std::string(names[k]) + " must be two characters");
            return SMI_ERR_INVALID;
        }
    if (cfg->table_log2 < 0 || cfg->table_log2 > 31) {
        set_error("smi_clipexport_config.table_log2 must be 0 .. 31");
        return SMI_ERR_INVALID;
    }
    SMI_HIP(hipSetDevice(ctx->device));
    smi_clipexport *h = new smi_clipexport();
    h->ctx = ctx;
    h->cfg = *cfg;
    hipError_t e = hipMalloc((void **)&h->d_words, W_COUNT * sizeof(unsigned long long));
    for (hipEvent_t &v : h->ev)
        if (e == hipSuccess) e = hipEventCreate(&v);
    if (e != hipSuccess) {
        clip_release(h);
        return hip_fail(e, "smi_clipexport_create");
    }
    *out = h;
    return SMI_OK;
}

extern "C" int smi_clipexport_free(smi_clipexport *h) {
    if (h) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        clip_release(h);
    }
    return SMI_OK;
}

extern "C" int smi_clipexport_counts(const smi_clipexport *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_clipexport_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof h->counts);
    return SMI_OK;
}

extern "C" int smi_clipexport_stage_ms(const smi_clipexport *h, float *ms) {
    if (!h || !ms) {
        set_error("smi_clipexport_stage_ms: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(ms, h->ms, sizeof h->ms);
    return SMI_OK;
}

extern "C" int smi_clipexport_error_read(const smi_clipexport *h, char *name, size_t cap, int64_t *record) {
    if (!h || !record || (cap && !name)) {
        set_error("smi_clipexport_error_read: null argument");
        return SMI_ERR_INVALID;
    }
    return handle::error_read(h->error_read, h->error_record, name, cap, record);
}

extern "C" int smi_clipexport_segment(smi_clipexport *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n, uint8_t *out,
                                      size_t cap, size_t *n_out) {
    if (!h || !n_out || n < 0 || (n && (!bam || !recs))) {
        set_error("smi_clipexport_segment: bad argument");
        return SMI_ERR_INVALID;
    }
    *n_out = 0;
    if (h->failed || h->dirty) {
        h->failed = true;
        set_error("smi_clipexport_segment: an earlier segment failed");
        return SMI_ERR_STATE;
    }
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    const size_t N = (size_t)n;
    const bool cached = h->last_n == n && h->last_bam == bam && h->last_recs == recs && h->last_n_bam == n_bam;
    h->last_n = -1;
    uint64_t total = 0;
    uint32_t winners = 0;
    if (cached) {
        total = h->last_total;
        winners = h->last_winners;
    } else {
        // every record inside the buffer, its attributes at its end: the kernels read nothing outside bam[0 .. n_bam) and the 4 bytes behind
        for (int32_t i = 0; i < n; i++) {
            const smi_bam_record &r = recs[i];
            if (r.rec_len < 36 || r.rec_off + r.rec_len > n_bam || r.name_off < r.rec_off || r.name_off + r.l_read_name > r.rec_off + r.rec_len ||
                r.cigar_off < r.rec_off || r.cigar_off + 4ull * r.n_cigar > r.rec_off + r.rec_len || r.aux_off < r.rec_off + 36 ||
                r.aux_off + r.aux_len != r.rec_off + r.rec_len) {
                set_error("smi_clipexport_segment: record index entry " + std::to_string(i) + " points outside the BAM buffer");
                return SMI_ERR_INVALID;
            }
        }
        // table entries and record numbers are uint32 with 0xffffffff for "none"; hipcub counts in int
        if ((uint64_t)h->resident + N > (uint64_t)INT32_MAX) {
            h->failed = true;
            set_error("ExportClippedReads: more than 2^31 - 1 written keys and records of one segment");
            return SMI_ERR_INVALID;
        }
        std::memset(h->ms, 0, sizeof h->ms);
        if (int rc = grow(&h->d_bam, h->bam_cap, n_bam + 8)) return rc;
        if (int rc = grow(&h->d_recs, h->recs_cap, N + 1)) return rc;
        if (int rc = grow(&h->d_cr, h->cr_cap, N + 1)) return rc;
        if (int rc = grow(&h->d_scan, h->scan_cap, 8 * (N + 1))) return rc;
        if (int rc = grow(&h->d_group, h->group_cap, N + 1)) return rc;
        if (int rc = grow(&h->d_first, h->first_cap, N + 1)) return rc;
        if (int rc = grow(&h->d_wlist, h->wlist_cap, N + 1)) return rc;
        if (int rc = grow(&h->d_decision, h->decision_cap, N + 1)) return rc;
        uint64_t *klen = h->d_scan, *koff = klen + (N + 1), *osize = koff + (N + 1), *ooff = osize + (N + 1), *rflag = ooff + (N + 1),
                 *rnew = rflag + (N + 1), *rsize = rnew + (N + 1), *rkoff = rsize + (N + 1);
        if (n_bam) SMI_HIP(hipMemcpyAsync(h->d_bam, bam, n_bam, hipMemcpyHostToDevice, s));
        SMI_HIP(hipMemcpyAsync(h->d_bam + n_bam, "null", 4, hipMemcpyHostToDevice, s));
        if (n) SMI_HIP(hipMemcpyAsync(h->d_recs, recs, N * sizeof(smi_bam_record), hipMemcpyHostToDevice, s));
        SMI_HIP(hipMemsetAsync(h->d_words, 0, W_COUNT * sizeof(unsigned long long), s));
        SMI_HIP(hipMemsetAsync(h->d_words + W_ERR, 0xFF, sizeof(unsigned long long), s));
        // K-CLIP-FLAG, the scan of the key lengths
        SMI_HIP(hipEventRecord(h->ev[0], s));
        {
            FlagArgs a = {};
            a.bam = h->d_bam;
            a.recs = h->d_recs;
            a.n = (uint32_t)n;
            const char *tags[kTags] = {h->cfg.gene_tag, h->cfg.cell_tag, h->cfg.umi_tag, h->cfg.us_tag, h->cfg.qs_tag};
            for (int k = 0; k < kTags; k++) a.key[k] = tag_key(tags[k]);
            a.min_clip = h->cfg.min_clip;
            a.null_off = n_bam;
            a.out = h->d_cr;
            a.klen = klen;
            a.words = h->d_words;
            hipLaunchKernelGGL(k_clip_flag, dim3(grid(N + 1)), dim3(kClipBlock), 0, s, a);
            SMI_HIP(hipGetLastError());
        }
        SMI_HIP(hipEventRecord(h->ev[1], s));
        unsigned long long words[W_COUNT] = {};
        uint64_t key_bytes = 0;
        SMI_HIP(hipMemcpyAsync(words, h->d_words, sizeof words, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipStreamSynchronize(s));
        h->ms[0] = elapsed(h->ev[0], h->ev[1]);
        if (words[W_BAD] & 1) {
            h->failed = true;
            set_error("smi_clipexport_segment: a record's attributes cannot be read: malformed or unknown attribute type");
            return SMI_ERR_INVALID;
        }
        const uint64_t clipped = words[W_CLIPPED];
        SMI_HIP(hipEventRecord(h->ev[0], s));
        if (int rc = clip_scan(h, s, klen, koff, N + 1)) return rc;
        SMI_HIP(hipMemcpyAsync(&key_bytes, koff + N, 8, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipStreamSynchronize(s));
        if (int rc = grow(&h->d_spool, h->spool_cap, (size_t)key_bytes + 1)) return rc;
        if (n) {
            hipLaunchKernelGGL(k_clip_key, dim3(grid(N)), dim3(kClipBlock), 0, s, (const uint8_t *)h->d_bam, (const smi_bam_record *)h->d_recs,
                               (const ClipRec *)h->d_cr, (const uint64_t *)koff, (uint32_t)n, h->d_spool);
            SMI_HIP(hipGetLastError());
        }
        SMI_HIP(hipEventRecord(h->ev[1], s));
        SMI_HIP(hipEventSynchronize(h->ev[1]));
        h->ms[1] = elapsed(h->ev[0], h->ev[1]);
        // K-CLIP-INSERT, K-CLIP-PICK, the three scans
        SMI_HIP(hipEventRecord(h->ev[0], s));
        if (int rc = clip_table(h, s, (uint64_t)h->resident + clipped)) return rc;
        SMI_HIP(hipMemsetAsync(h->d_first, 0xff, (N + 1) * sizeof(uint32_t), s));
        h->dirty = true;
        if (n) {
            InsArgs a = {h->d_rpool, h->d_roff, h->d_spool, koff, h->resident, (uint32_t)n, (uint32_t)(h->slots - 1), h->d_tab, h->d_group, h->d_first,
                         h->d_words};
            hipLaunchKernelGGL(k_clip_insert, dim3(grid(N)), dim3(kClipBlock), 0, s, a);
            SMI_HIP(hipGetLastError());
        }
        {
            PickArgs a = {h->d_cr, h->d_group, h->d_first, h->resident, (uint32_t)n, osize, rflag, rsize, h->d_wlist, h->d_decision, h->d_words};
            hipLaunchKernelGGL(k_clip_pick, dim3(grid(N + 1)), dim3(kClipBlock), 0, s, a);
            SMI_HIP(hipGetLastError());
        }
        if (int rc = clip_scan(h, s, osize, ooff, N + 1)) return rc;
        if (int rc = clip_scan(h, s, rflag, rnew, N + 1)) return rc;
        if (int rc = clip_scan(h, s, rsize, rkoff, N + 1)) return rc;
        uint64_t n_new = 0, new_bytes = 0;
        SMI_HIP(hipMemcpyAsync(words, h->d_words, sizeof words, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipMemcpyAsync(&total, ooff + N, 8, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipMemcpyAsync(&n_new, rnew + N, 8, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipMemcpyAsync(&new_bytes, rkoff + N, 8, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipStreamSynchronize(s));
        if (words[W_ERR] != kNoRecord) {  // the reference's loop ends at this record and leaves a cut-off file: the run stops here
            h->failed = true;
            const smi_bam_record &r = recs[words[W_ERR]];
            ClipRec c;
            SMI_HIP(hipMemcpy(&c, h->d_cr + words[W_ERR], sizeof c, hipMemcpyDeviceToHost));
            h->error_read.assign((const char *)bam + r.name_off, r.l_read_name ? r.l_read_name - 1u : 0u);
            h->error_record = h->counts[SMI_CLIP_RECORDS] + (int64_t)words[W_ERR];
            set_error("read " + h->error_read + ": " + kStopText[std::min<uint32_t>(c.flags >> CLIP_KIND_SHIFT, 4u)]);
            return 2;
        }
        if (words[W_BAD] & 2) {  // (cannot happen: the table is at most half full)
            h->failed = true;
            set_error("ExportClippedReads: the K-CLIP-INSERT table ran full");
            return SMI_ERR_STATE;
        }
        winners = (uint32_t)words[W_WINNERS];
        // K-CLIP-COMMIT
        if (n_new) {
            if (int rc = grow_keep(&h->d_rpool, h->rpool_cap, (size_t)h->resident_bytes, (size_t)(h->resident_bytes + new_bytes) + 1, s)) return rc;
            if (int rc = grow_keep(&h->d_roff, h->roff_cap, (size_t)h->resident + 1, (size_t)h->resident + n_new + 2, s)) return rc;
            hipLaunchKernelGGL(k_clip_commit, dim3(grid(N + 1)), dim3(kClipBlock), 0, s, (const uint64_t *)rflag, (const uint64_t *)rnew,
                               (const uint64_t *)rkoff, (const uint8_t *)h->d_spool, (const uint64_t *)koff, (uint32_t)n, h->resident, h->resident_bytes,
                               h->d_rpool, h->d_roff);
            hipLaunchKernelGGL(k_clip_remap, dim3(grid(h->slots)), dim3(kClipBlock), 0, s, h->d_tab, (uint32_t)h->slots, h->resident, (const uint64_t *)rnew);
            SMI_HIP(hipGetLastError());
            h->resident += (uint32_t)n_new;
            h->resident_bytes += new_bytes;
        }
        SMI_HIP(hipEventRecord(h->ev[1], s));
        std::vector<uint8_t> decision;
        if (h->cfg.keep_records && n) {
            decision.resize(N);
            SMI_HIP(hipMemcpyAsync(decision.data(), h->d_decision, N, hipMemcpyDeviceToHost, s));
        }
        SMI_HIP(hipStreamSynchronize(s));
        h->dirty = false;
        h->ms[2] = elapsed(h->ev[0], h->ev[1]);
        h->counts[SMI_CLIP_RECORDS] += n;
        h->counts[SMI_CLIP_CLIPPED] += (int64_t)clipped;
        h->counts[SMI_CLIP_WRITTEN] += winners;
        h->counts[SMI_CLIP_SEGMENTS]++;
        h->counts[SMI_CLIP_PROBE_STEPS] += (int64_t)words[W_STEPS];
        h->counts[SMI_CLIP_WRAPS] += (int64_t)words[W_WRAPS];
        if (h->cfg.keep_records) {
            const uint16_t keys[3] = {lr::tag16(h->cfg.gene_tag), lr::tag16(h->cfg.cell_tag), lr::tag16(h->cfg.umi_tag)};
            for (int32_t i = 0; i < n; i++) {
                const smi_bam_record &r = recs[i];
                smi_clipexport::Kept k;
                k.name.assign((const char *)bam + r.name_off, r.l_read_name ? r.l_read_name - 1u : 0u);
                k.has[0] = k.has[1] = k.has[2] = 0;
                const uint8_t *p = bam + r.aux_off, *end = p + r.aux_len;
                size_t sz = 0;
                while (p < end && lr::aux_size(p, end, &sz) == 0) {
                    for (int t = 0; t < 3; t++)
                        if ((uint16_t)(p[0] | p[1] << 8) == keys[t]) {
                            k.has[t] = 1;
                            k.tag[t].assign((const char *)p + 3, sz - 4);
                        }
                    p += sz;
                }
                k.cigar.resize(r.n_cigar);
                if (r.n_cigar) std::memcpy(k.cigar.data(), bam + r.cigar_off, 4ull * r.n_cigar);
                k.decision = decision[(size_t)i];
                h->kept.push_back(std::move(k));
            }
        }
    }
    *n_out = total;
    if (!out || cap < total) {  // sizes only: the segment stays on the device for the next call with the same arguments
        h->last_bam = bam;
        h->last_recs = recs;
        h->last_n_bam = n_bam;
        h->last_n = n;
        h->last_total = total;
        h->last_winners = winners;
        return out ? 1 : SMI_OK;
    }
    if (!total) return SMI_OK;
    // K-CLIP-WRITE
    if (int rc = grow(&h->d_out, h->out_cap, (size_t)total)) return rc;
    const uint64_t *koff = h->d_scan + (N + 1), *ooff = h->d_scan + 3 * (N + 1);
    SMI_HIP(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(k_clip_write, dim3(blocks_for(winners, kClipWaves)), dim3(64 * kClipWaves), 0, s, (const uint8_t *)h->d_bam,
                       (const ClipRec *)h->d_cr, (const uint32_t *)h->d_wlist, winners, (const uint8_t *)h->d_spool, koff, ooff, h->d_out, (uint64_t)total);
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipEventRecord(h->ev[1], s));
    SMI_HIP(hipMemcpyAsync(out, h->d_out, total, hipMemcpyDeviceToHost, s));
    SMI_HIP(hipStreamSynchronize(s));
    h->ms[3] = elapsed(h->ev[0], h->ev[1]);
    return SMI_OK;
}

// the reference's loop as it runs it (ExportClippedReads.java:L64-96): one thread, a hash set of the keys written, over the records the
// segments handed in (keep_records)
extern "C" int smi_clipexport_host_loop(const smi_clipexport *h, double *seconds, int64_t *mismatches) {
    if (!h || !seconds || !mismatches) {
        set_error("smi_clipexport_host_loop: null argument");
        return SMI_ERR_INVALID;
    }
    if (!h->cfg.keep_records || h->failed) {
        set_error(h->failed ? "smi_clipexport_host_loop: a segment failed" : "smi_clipexport_host_loop: the handle was created without keep_records");
        return SMI_ERR_STATE;
    }
    static const char ops[] = "MIDNSHP=XBBBBBBB";
    const auto t0 = std::chrono::steady_clock::now();
    std::unordered_set<std::string> written;
    std::vector<uint8_t> mine(h->kept.size());
    std::string key, cigar;
    for (size_t i = 0; i < h->kept.size(); i++) {
        const smi_clipexport::Kept &k = h->kept[i];
        const std::vector<std::string_view> tmp = lr::jsplit(k.name, '_');
        key.assign(tmp.empty() ? std::string_view() : tmp[0]);
        for (int t = 0; t < 3; t++) {
            key += '_';
            key += k.has[t] ? k.tag[t] : std::string("null");
        }
        cigar.clear();
        for (uint32_t c : k.cigar) {
            cigar += std::to_string(c >> 4);
            cigar += ops[c & 15];
        }
        bool clipped = false;
        if (!cigar.empty()) {
            size_t d = 0;
            while (d < cigar.size() && cigar[d] >= '0' && cigar[d] <= '9') d++;
            if ((cigar[d] == 'H' || cigar[d] == 'S') && std::stoll(cigar.substr(0, d)) > h->cfg.min_clip) clipped = true;
            const char last = cigar.back();
            size_t b = cigar.size() - 1;
            while (b > 0 && cigar[b - 1] >= '0' && cigar[b - 1] <= '9') b--;
            if ((last == 'H' || last == 'S') && std::stoll(cigar.substr(b, cigar.size() - 1 - b)) > h->cfg.min_clip) clipped = true;
        }
        bool wrote = false;
        if (clipped && !written.count(key)) {
            wrote = true;
            written.insert(key);
        }
        mine[i] = (uint8_t)((clipped ? 1 : 0) | (wrote ? 2 : 0));
    }
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    int64_t bad = 0;
    for (size_t i = 0; i < h->kept.size(); i++) bad += mine[i] != h->kept[i].decision;
    *mismatches = bad;
    return SMI_OK;
}
