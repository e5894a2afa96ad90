// smi_tagbam.hip -- K-TAG: `tagbamwithread` (FJ!com/rw/tagbamwithread/TagWithReadSequenceMain.java:L85-116) on the device.
//
// The reference keeps a HashMap<read name, FastqRecord> per chromosome (ReadNameChrHashMap.getFastqsForChromosome L85-106, fed by
// SplitFastqByChromosome.split L45-92 through a temporary FASTQ per chromosome) and, per BAM record in file order, drops the record
// without a reference, reports and drops the record whose name the map lacks, and otherwise setAttribute(readTag, bases) /
// setAttribute(qvTag, qualities) + addSam.  Every lookup gives what ONE global map gives whose key is getReadName().split(" ")[0] and
// where a name that occurs twice keeps its LAST record (put overwrites).  Here:
//   K-TAG-KEY   one thread per FASTQ record (K-FQ's index): token length (up to the first ' ') and a 64-bit hash of the token
//   K-TAG-BUILD one thread per record: open addressing over 2^k >= 2n slots of `tag << 32 | record index`; an empty slot is claimed by
//               CAS, a slot with the same tag is compared byte for byte in the resident FASTQ text and, for the same token, atomicMax'ed:
//               the highest index (the last record) wins whatever order the threads arrive in
//   K-TAG-PROBE one thread per BAM record: UNMAPPED (reference index -1), the FASTQ record, or MISSING; every tag hit is confirmed
//               byte for byte
//   K-TAG-ASM   one wavefront per BAM record: k_aux_rewrite<WRITE, TagSource> of smi_auxedit.h, the attribute rewrite shared with K-EDIT
//               (smi_moltag.hip), as SIZE + exclusive scan + WRITE through an AuxRewriter.  TagSource drops the records K-TAG-PROBE did not
//               find (before their attributes are read) and puts two Z fields behind the others, their payloads copied straight from the
//               FASTQ text.  tag_assemble_z2 runs the same kernel for IsoformMatrix's ISOBAM (smi_isoform.hip).
// The attribute rules (htsjdk's, pinned by tests/golden/ref_exec_auxorder.json) are stated in smi_auxedit.h.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "smi_auxedit.h"
#include "smi_internal.h"

namespace smi {
namespace {

constexpr uint64_t kEmpty = ~0ull;          // no valid entry: record indices stay below 2^31
constexpr int32_t kMissing = -1, kUnmapped = -2;

__device__ __forceinline__ uint64_t mix64(uint64_t h) {  // splitmix64's finaliser
    h ^= h >> 30;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27;
    h *= 0x94d049bb133111ebull;
    return h ^ (h >> 31);
}
__device__ __forceinline__ uint64_t hash_bytes(const uint8_t *p, uint32_t n, uint64_t hash_mask) {
    uint64_t h = kFnvBasis ^ n;  // FNV-1a over the bytes, then mixed
    for (uint32_t i = 0; i < n; i++) h = fnv1a_add(h, p[i]);
    return mix64(h) & hash_mask;
}

__global__ void k_tag_key(const uint8_t *__restrict__ text, const uint64_t *__restrict__ name_start, const uint32_t *__restrict__ name_len,
                          size_t n, uint64_t hash_mask, uint32_t *__restrict__ key_len, uint64_t *__restrict__ hash) {
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint8_t *p = text + name_start[r];
    const uint32_t len = name_len[r];
    uint32_t k = 0;
    while (k < len && p[k] != ' ') k++;  // getReadName().split(" ")[0]: a tab stays in the key
    key_len[r] = k;
    hash[r] = hash_bytes(p, k, hash_mask);
}

__global__ void k_tag_build(const uint8_t *__restrict__ text, const uint64_t *__restrict__ name_start, const uint32_t *__restrict__ key_len,
                            const uint64_t *__restrict__ hash, size_t n, unsigned long long *__restrict__ table, uint64_t mask) {
    const size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint64_t h = hash[r];
    const unsigned long long mine = (h >> 32) << 32 | (uint64_t)r;
    const uint8_t *key = text + name_start[r];
    const uint32_t klen = key_len[r];
    uint64_t s = h & mask;
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {  // the table is never full (>= 2n slots): the loop ends at an empty slot
        unsigned long long w = table[s];
        if (w == kEmpty) {
            w = atomicCAS(&table[s], (unsigned long long)kEmpty, mine);
            if (w == kEmpty) return;
        }
        if ((w >> 32) != (h >> 32)) continue;
        const uint32_t o = (uint32_t)w;  // same tag: the same token? (a slot never changes its token once claimed)
        if (key_len[o] == klen && same_bytes(text + name_start[o], key, klen)) {
            atomicMax(&table[s], mine);  // last record wins
            return;
        }
    }
}

__global__ void k_tag_probe(const uint8_t *__restrict__ bam, const smi_bam_record *__restrict__ recs, size_t n, const uint8_t *__restrict__ text,
                            const uint64_t *__restrict__ name_start, const uint32_t *__restrict__ key_len, const uint64_t *__restrict__ table,
                            uint64_t mask, uint64_t hash_mask, int32_t *__restrict__ res) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const smi_bam_record rec = recs[i];
    if (rec.ref_id == -1) {  // getReferenceName() == "*": dropped (L92-94)
        res[i] = kUnmapped;
        return;
    }
    const uint8_t *nm = bam + rec.name_off;
    const uint32_t len = rec.l_read_name ? rec.l_read_name - 1u : 0u;
    const uint64_t h = hash_bytes(nm, len, hash_mask);
    int32_t found = kMissing;
    uint64_t s = h & mask;
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint64_t w = table[s];
        if (w == kEmpty) break;
        if ((w >> 32) != (h >> 32)) continue;
        const uint32_t o = (uint32_t)w;
        if (key_len[o] == len && same_bytes(text + name_start[o], nm, len)) {
            found = (int32_t)o;
            break;
        }
    }
    res[i] = found;
}

// what K-TAG-ASM puts behind a record's own attributes: two Z fields whose payloads lie in the resident text (the second one optional)
struct TagSource {
    const int32_t *res;  // per record: the entry of its payloads, or negative: the record is dropped
    const uint8_t *text;
    const uint64_t *a_start, *b_start;
    const uint32_t *a_len, *b_len;
    uint32_t a_key, b_key;
    int with_b;
    struct Tail {
        Field a, b;
        bool with_b;
        __device__ uint32_t put(Field *f, int &n) const { return put_field(f, n, a) && (!with_b || put_field(f, n, b)) ? 0 : SMI_TAG_TOO_MANY_ATTRS; }
    };
    __device__ bool keeps(size_t i) const { return res[i] >= 0; }
    __device__ Tail tail(size_t i) const {
        const int32_t k = res[i];
        return {{(uint16_t)a_key, 3, 0, a_len[k], a_start[k], 0, 0}, {(uint16_t)b_key, 3, 0, b_len[k], b_start[k], 0, 0}, with_b != 0};
    }
    __device__ const uint8_t *payload() const { return text; }
};

}  // namespace

// K-TAG-ASM for records already on the device (smi_internal.h)
int tag_assemble_z2(hipStream_t s, const uint8_t *d_bam, const smi_bam_record *d_recs, size_t n, const int32_t *d_entry, const uint8_t *d_text,
                    const uint64_t *d_a_start, const uint32_t *d_a_len, const uint64_t *d_b_start, const uint32_t *d_b_len, const char *tag_a,
                    const char *tag_b, std::vector<uint8_t> &out, float *ms) {
    out.clear();
    if (!n) return SMI_OK;
    const TagSource src = {d_entry, d_text, d_a_start, d_b_start, d_a_len, d_b_len, tag_key(tag_a), tag_key(tag_b), 1};
    AuxRewriter rw;
    uint64_t total = 0;
    float t_size = 0.f, t_write = 0.f;
    if (int rc = rw.size("", s, d_bam, d_recs, n, src, &total, &t_size)) return rc;
    out.resize(total);
    if (total)
        if (int rc = rw.write("", s, d_bam, d_recs, n, src, total, out.data(), &t_write)) return rc;
    if (ms) *ms += t_size + t_write;
    return SMI_OK;
}

}  // namespace smi

using namespace smi;

struct smi_tagbam {
    smi_ctx *ctx = nullptr;
    smi_tagbam_config cfg = {};
    uint64_t hash_mask = ~0ull;
    uint8_t *d_text = nullptr;
    size_t n_text = 0, n_fq = 0;
    uint64_t *d_line_start = nullptr, *d_name_start = nullptr, *d_seq_start = nullptr, *d_qual_start = nullptr, *d_offsets = nullptr;
    uint32_t *d_name_len = nullptr, *d_seq_len = nullptr, *d_key_len = nullptr;
    uint64_t *d_table = nullptr;
    uint64_t mask = 0;
    // one segment (grow-only)
    uint8_t *d_bam = nullptr;
    size_t bam_cap = 0;
    smi_bam_record *d_recs = nullptr;
    int32_t *d_res = nullptr;
    size_t recs_cap = 0, res_cap = 0;
    AuxRewriter rw;  // K-TAG-ASM: SIZE + scan, WRITE
    std::vector<int32_t> res;
    // the segment the last call sized and did not write (out too small / NULL): the next call with the same arguments writes it
    const uint8_t *last_bam = nullptr;
    const smi_bam_record *last_recs = nullptr;
    size_t last_n_bam = 0;
    int32_t last_n = -1;
    uint64_t last_total = 0;
    hipEvent_t ev[4] = {};
    float ms[SMI_TAGBAM_STAGES] = {};
};

namespace {

void tagbam_release(smi_tagbam *h) {
    void *bufs[] = {h->d_text, h->d_line_start, h->d_name_start, h->d_seq_start, h->d_qual_start, h->d_offsets, h->d_name_len, h->d_seq_len,
                    h->d_key_len, h->d_table, h->d_bam, h->d_recs, h->d_res};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
}

// the read (and QV) attribute of the record whose FASTQ entry K-TAG-PROBE found
TagSource tag_source(const smi_tagbam *h) {
    return {h->d_res, h->d_text, h->d_seq_start, h->d_qual_start, h->d_seq_len, h->d_seq_len, tag_key(h->cfg.read_tag), tag_key(h->cfg.qv_tag),
            h->cfg.with_qv};
}

}  // namespace

extern "C" int smi_tagbam_default_config(smi_tagbam_config *cfg) {
    if (!cfg) {
        set_error("smi_tagbam_default_config: null argument");
        return SMI_ERR_INVALID;
    }
    *cfg = {};
    std::memcpy(cfg->read_tag, "US", 3);
    std::memcpy(cfg->qv_tag, "QS", 3);
    return SMI_OK;
}

extern "C" int smi_tagbam_create(smi_ctx *ctx, const uint8_t *fastq_text, size_t n_bytes, const smi_tagbam_config *cfg, smi_tagbam **out,
                                 uint32_t *errors) {
    if (!ctx || !cfg || !out || !errors || (n_bytes && !fastq_text)) {
        set_error("smi_tagbam_create: null argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    *errors = 0;
    if (!valid_tag(cfg->read_tag)) {
        set_error("read tag must be two characters");
        return SMI_ERR_INVALID;
    }
    if (cfg->with_qv && !valid_tag(cfg->qv_tag)) {
        set_error("QV tag must be two characters");
        return SMI_ERR_INVALID;
    }
    if (cfg->hash_bits < 0 || cfg->hash_bits > 64) {
        set_error("smi_tagbam_create: hash_bits must be 0 .. 64");
        return SMI_ERR_INVALID;
    }
    if (n_bytes >= ((size_t)1 << 42)) {
        set_error("smi_tagbam_create: FASTQ text of " + std::to_string(n_bytes) + " bytes is larger than one index takes (2^42)");
        return SMI_ERR_INVALID;
    }
    SMI_HIP(hipSetDevice(ctx->device));
    smi_tagbam *h = new smi_tagbam();
    h->ctx = ctx;
    h->cfg = *cfg;
    h->hash_mask = cfg->hash_bits == 0 || cfg->hash_bits == 64 ? ~0ull : (1ull << cfg->hash_bits) - 1;
    hipStream_t s = ctx->stream;
    auto fail = [&](int rc) {
        tagbam_release(h);
        return rc;
    };
#define TAG_HIP(call)                                            \
    do {                                                         \
        hipError_t e__ = (call);                                 \
        if (e__ != hipSuccess) return fail(hip_fail(e__, #call)); \
    } while (0)
    for (hipEvent_t &e : h->ev) TAG_HIP(hipEventCreate(&e));
    // the whole text stays on the device (the Z payloads are copied from it): refuse a text that does not fit, with the sizes, before any kernel
    size_t free_b = 0, total_b = 0;
    TAG_HIP(hipMemGetInfo(&free_b, &total_b));
    {
        const size_t est = n_bytes + 1 + (n_bytes / 4 + 2) * 8;  // text + the line table, needed before the record count is known
        if (est > free_b) {
            set_error("smi_tagbam_create: FASTQ text of " + std::to_string(n_bytes) + " bytes needs at least " + std::to_string(est) +
                      " bytes of device memory, " + std::to_string(free_b) + " of " + std::to_string(total_b) + " are free");
            return fail(SMI_ERR_INVALID);
        }
    }
    TAG_HIP(hipMalloc(&h->d_text, n_bytes + 1));
    h->n_text = n_bytes;
    if (n_bytes) TAG_HIP(hipMemcpyAsync(h->d_text, fastq_text, n_bytes, hipMemcpyHostToDevice, s));
    size_t n_lines = 0;
    if (n_bytes) {
        if (int rc = launch_fastq_sweep(ctx, h->d_text, n_bytes, &n_lines, s)) return fail(rc);
    }
    const size_t cap_lines = n_lines + 2, cap_rec = n_lines / 4 + 2;
    {
        const size_t table_slots = std::max<size_t>(64, (size_t)1 << (64 - __builtin_clzll((unsigned long long)(2 * cap_rec - 1))));
        const size_t need = cap_lines * 8 + cap_rec * (5 * 8 + 3 * 4) + table_slots * 8;
        TAG_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b) {
            set_error("smi_tagbam_create: FASTQ of " + std::to_string(n_bytes) + " bytes / " + std::to_string(n_lines / 4) + " records needs " +
                      std::to_string(need) + " bytes of device memory beside its text, " + std::to_string(free_b) + " of " + std::to_string(total_b) +
                      " are free");
            return fail(SMI_ERR_INVALID);
        }
        h->mask = table_slots - 1;
    }
    TAG_HIP(hipMalloc(&h->d_line_start, cap_lines * 8));
    TAG_HIP(hipMalloc(&h->d_name_start, cap_rec * 8));
    TAG_HIP(hipMalloc(&h->d_seq_start, cap_rec * 8));
    TAG_HIP(hipMalloc(&h->d_qual_start, cap_rec * 8));
    TAG_HIP(hipMalloc(&h->d_offsets, cap_rec * 8));
    TAG_HIP(hipMalloc(&h->d_name_len, cap_rec * 4));
    TAG_HIP(hipMalloc(&h->d_seq_len, cap_rec * 4));
    TAG_HIP(hipMalloc(&h->d_key_len, cap_rec * 4));
    TAG_HIP(hipMalloc(&h->d_table, (h->mask + 1) * 8));
    size_t n_fq = 0;
    uint32_t fq_err = 0;
    if (n_bytes) {
        if (int rc = launch_fastq_index(ctx, h->d_text, n_bytes, h->d_line_start, cap_lines, h->d_name_start, h->d_name_len, h->d_seq_start,
                                        h->d_seq_len, h->d_qual_start, h->d_offsets, cap_rec, &n_fq, &fq_err, s))
            return fail(rc);
    }
    if (fq_err) {  // htsjdk's FastqReader throws on the same text: reported, never repaired
        *errors = fq_err;
        set_error(std::string("FASTQ text is malformed:") + (fq_err & SMI_FQ_BAD_SEQ_HEADER ? " a record's first line does not start with '@';" : "") +
                  (fq_err & SMI_FQ_BAD_QUAL_HEADER ? " a record's third line does not start with '+';" : "") +
                  (fq_err & SMI_FQ_LENGTH_MISMATCH ? " sequence and quality lines differ in length;" : "") +
                  (fq_err & SMI_FQ_TRUNCATED ? " the text does not end on a record boundary;" : ""));
        return fail(SMI_ERR_INVALID);
    }
    h->n_fq = n_fq;
    TAG_HIP(hipMemsetAsync(h->d_table, 0xFF, (h->mask + 1) * 8, s));
    // the hashes live in the line table, which the index no longer needs (cap_lines >= n_fq)
    uint64_t *d_hash = h->d_line_start;
    TAG_HIP(hipEventRecord(h->ev[0], s));
    if (n_fq)
        hipLaunchKernelGGL(k_tag_key, dim3(blocks_for(n_fq, 256)), dim3(256), 0, s, (const uint8_t *)h->d_text, (const uint64_t *)h->d_name_start,
                           (const uint32_t *)h->d_name_len, n_fq, h->hash_mask, h->d_key_len, d_hash);
    TAG_HIP(hipGetLastError());
    TAG_HIP(hipEventRecord(h->ev[1], s));
    if (n_fq)
        hipLaunchKernelGGL(k_tag_build, dim3(blocks_for(n_fq, 256)), dim3(256), 0, s, (const uint8_t *)h->d_text, (const uint64_t *)h->d_name_start,
                           (const uint32_t *)h->d_key_len, (const uint64_t *)d_hash, n_fq, (unsigned long long *)h->d_table, h->mask);
    TAG_HIP(hipGetLastError());
    TAG_HIP(hipEventRecord(h->ev[2], s));
    TAG_HIP(hipStreamSynchronize(s));
    h->ms[0] = elapsed(h->ev[0], h->ev[1]);
    h->ms[1] = elapsed(h->ev[1], h->ev[2]);
#undef TAG_HIP
    *out = h;
    return SMI_OK;
}

extern "C" int smi_tagbam_free(smi_tagbam *h) {
    if (h) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        tagbam_release(h);
    }
    return SMI_OK;
}

extern "C" int smi_tagbam_records(const smi_tagbam *h, size_t *n_records) {
    if (!h || !n_records) {
        set_error("smi_tagbam_records: null argument");
        return SMI_ERR_INVALID;
    }
    *n_records = h->n_fq;
    return SMI_OK;
}

extern "C" int smi_tagbam_stage_ms(const smi_tagbam *h, float *ms) {
    if (!h || !ms) {
        set_error("smi_tagbam_stage_ms: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(ms, h->ms, sizeof h->ms);
    return SMI_OK;
}

extern "C" int smi_tagbam_segment(smi_tagbam *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n, uint8_t *out, size_t cap,
                                  size_t *n_out, int32_t *missing, int32_t *n_missing, int32_t *n_unmapped) {
    if (!h || !n_out || !n_missing || !n_unmapped || n < 0 || (n && (!bam || !recs || !missing))) {
        set_error("smi_tagbam_segment: bad argument");
        return SMI_ERR_INVALID;
    }
    *n_out = 0;
    *n_missing = *n_unmapped = 0;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    const bool cached = h->last_n == n && h->last_bam == bam && h->last_recs == recs && h->last_n_bam == n_bam;
    h->last_n = -1;
    uint64_t total = 0;
    if (cached) {
        total = h->last_total;
    } else {
        // every record inside the buffer, its attributes at its end: the kernels read nothing outside bam[0 .. n_bam)
        for (int32_t i = 0; i < n; i++) {
            const smi_bam_record &r = recs[i];
            if (r.rec_len < 36 || r.rec_off + r.rec_len > n_bam || r.name_off + r.l_read_name > n_bam || r.aux_off < r.rec_off + 36 ||
                r.aux_off + r.aux_len != r.rec_off + r.rec_len) {
                set_error("smi_tagbam_segment: record index entry " + std::to_string(i) + " points outside the BAM buffer");
                return SMI_ERR_INVALID;
            }
        }
        if (int rc = grow(&h->d_bam, h->bam_cap, n_bam + 1)) return rc;
        if (int rc = grow(&h->d_recs, h->recs_cap, (size_t)n + 1)) return rc;
        if (int rc = grow(&h->d_res, h->res_cap, (size_t)n + 1)) return rc;
        if (n_bam) SMI_HIP(hipMemcpyAsync(h->d_bam, bam, n_bam, hipMemcpyHostToDevice, s));
        if (n) SMI_HIP(hipMemcpyAsync(h->d_recs, recs, (size_t)n * sizeof(smi_bam_record), hipMemcpyHostToDevice, s));
        SMI_HIP(hipEventRecord(h->ev[2], s));
        if (n)
            hipLaunchKernelGGL(k_tag_probe, dim3(blocks_for(n, 256)), dim3(256), 0, s, (const uint8_t *)h->d_bam, (const smi_bam_record *)h->d_recs,
                               (size_t)n, (const uint8_t *)h->d_text, (const uint64_t *)h->d_name_start, (const uint32_t *)h->d_key_len,
                               (const uint64_t *)h->d_table, h->mask, h->hash_mask, h->d_res);
        SMI_HIP(hipGetLastError());
        SMI_HIP(hipEventRecord(h->ev[3], s));
        h->res.resize((size_t)n + 1);
        const int rc = h->rw.size("smi_tagbam_segment: ", s, h->d_bam, h->d_recs, (size_t)n, tag_source(h), &total, &h->ms[3], [&] {
            return n ? hipMemcpyAsync(h->res.data(), h->d_res, (size_t)n * 4, hipMemcpyDeviceToHost, s) : hipSuccess;  // read back on size()'s wait
        });
        h->ms[2] = elapsed(h->ev[2], h->ev[3]);
        if (rc) return rc;
    }
    int32_t nm = 0, nu = 0;
    for (int32_t i = 0; i < n; i++) {
        if (h->res[i] == kUnmapped)
            nu++;
        else if (h->res[i] == kMissing)
            missing[nm++] = i;
    }
    *n_missing = nm;
    *n_unmapped = nu;
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
    return h->rw.write("smi_tagbam_segment: ", s, h->d_bam, h->d_recs, (size_t)n, tag_source(h), total, out, &h->ms[4]);
}
