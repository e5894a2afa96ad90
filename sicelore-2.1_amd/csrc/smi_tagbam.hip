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
//   K-TAG-ASM   one wavefront per BAM record, in two instantiations: SIZE (lane 0 parses the attributes and sizes the record) and
//               WRITE (lane 0 parses into LDS; the wavefront copies the fixed part, the attributes and the two Z payloads straight from
//               the FASTQ text into the output at the offset of the exclusive scan of the sizes)
// The attribute list is what htsjdk writes after setAttribute (BinaryTagCodec.readTags L271-305 + SAMBinaryTagAndValue.insert L207-228,
// pinned by tests/golden/ref_exec_auxorder.json): ordered by binary tag, a repeated tag keeping its last value, integers in the smallest
// type (getIntegerType L153-180), H read back as a byte array (B:c).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "smi_internal.h"

namespace smi {
namespace {

constexpr uint64_t kEmpty = ~0ull;          // no valid entry: record indices stay below 2^31
constexpr int32_t kMissing = -1, kUnmapped = -2;
constexpr int kMaxFields = SMI_TAGBAM_MAX_ATTRS;
constexpr int kAsmWaves = 4;                // waves per block of K-TAG-ASM

__device__ __forceinline__ uint64_t mix64(uint64_t h) {  // splitmix64's finaliser
    h ^= h >> 30;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27;
    h *= 0x94d049bb133111ebull;
    return h ^ (h >> 31);
}
__device__ __forceinline__ uint64_t hash_bytes(const uint8_t *p, uint32_t n, uint64_t hash_mask) {
    uint64_t h = 0xcbf29ce484222325ull ^ n;  // FNV-1a over the bytes, then mixed
    for (uint32_t i = 0; i < n; i++) h = (h ^ p[i]) * 0x100000001b3ull;
    return mix64(h) & hash_mask;
}
__device__ __forceinline__ bool same_bytes(const uint8_t *a, const uint8_t *b, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (a[i] != b[i]) return false;
    return true;
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

// one attribute of the written record
struct Field {
    uint16_t key;    // binary tag: second char << 8 | first char (SAMTag.makeBinaryTag L124-127)
    uint8_t kind;    // 0 verbatim (src: type byte .. end), 1 integer (ival), 2 H -> B:c (src: the hex digits), 3 Z from the FASTQ text
    uint8_t type;    // output type of an integer
    uint32_t len;    // kind 0: bytes behind the tag; 2: hex digits; 3: payload bytes
    uint64_t src;    // kind 0 / 2: offset in the BAM stream; 3: offset in the FASTQ text
    int64_t ival;
    uint64_t out;    // offset of the field in the output record (WRITE)
};

__device__ __forceinline__ uint32_t field_bytes(const Field &f) {
    switch (f.kind) {
        case 1: return 3u + (f.type == 'c' || f.type == 'C' ? 1u : f.type == 's' || f.type == 'S' ? 2u : 4u);
        case 2: return 8u + f.len / 2;
        case 3: return 4u + f.len;
        default: return 2u + f.len;
    }
}
__device__ __forceinline__ uint8_t int_type(int64_t v) {  // BinaryTagCodec.getIntegerType
    if (v >= -128 && v <= 127) return 'c';
    if (v >= 0 && v <= 255) return 'C';
    if (v >= -32768 && v <= 32767) return 's';
    if (v >= 0 && v <= 65535) return 'S';
    if (v >= -2147483648ll && v <= 2147483647ll) return 'i';
    return 'I';
}
__device__ __forceinline__ int hex_val(uint8_t c) {
    if (c >= '0' && c <= '9') return c - '0';
    c |= 0x20;
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}
__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// insert or replace (a repeated tag keeps its last value); false: more than kMaxFields attributes
__device__ bool put_field(Field *f, int &n, const Field &x) {
    for (int j = 0; j < n; j++)
        if (f[j].key == x.key) {
            f[j] = x;
            return true;
        }
    if (n >= kMaxFields) return false;
    f[n++] = x;
    return true;
}

// lane 0: the attribute list of record rec as written, in f[0 .. n), sorted by binary tag; returns SMI_TAG_* error bits (0 = fine)
__device__ uint32_t parse_fields(const uint8_t *__restrict__ bam, const smi_bam_record &rec, const uint8_t *__restrict__ text, uint64_t seq_start,
                                 uint64_t qual_start, uint32_t seq_len, uint32_t qual_len, uint32_t read_key, uint32_t qv_key, bool with_qv, Field *f,
                                 int &n) {
    n = 0;
    const uint64_t end = rec.aux_off + rec.aux_len;
    uint64_t p = rec.aux_off;
    while (p < end) {
        if (p + 3 > end) return SMI_TAG_BAD_AUX;
        Field x = {};
        x.key = (uint16_t)(bam[p + 1] << 8 | bam[p]);
        const uint8_t ty = bam[p + 2];
        const uint64_t v = p + 3;
        uint64_t q;
        switch (ty) {
            case 'A': q = v + 1; break;
            case 'f': q = v + 4; break;
            case 'c': case 'C': case 's': case 'S': case 'i': case 'I': {
                const uint32_t w = ty == 'c' || ty == 'C' ? 1 : ty == 's' || ty == 'S' ? 2 : 4;
                q = v + w;
                if (q > end) return SMI_TAG_BAD_AUX;
                const uint32_t raw = w == 1 ? bam[v] : w == 2 ? (uint32_t)(bam[v] | bam[v + 1] << 8) : ld_u32(bam + v);
                x.kind = 1;
                x.ival = ty == 'c' ? (int64_t)(int8_t)raw : ty == 's' ? (int64_t)(int16_t)raw : ty == 'i' ? (int64_t)(int32_t)raw : (int64_t)raw;
                x.type = int_type(x.ival);
                break;
            }
            case 'Z': case 'H': {
                q = v;
                while (q < end && bam[q]) q++;
                if (q >= end) return SMI_TAG_BAD_AUX;
                if (ty == 'H') {
                    const uint32_t digits = (uint32_t)(q - v);
                    if (digits & 1u) return SMI_TAG_BAD_HEX;
                    for (uint64_t k = v; k < q; k++)
                        if (hex_val(bam[k]) < 0) return SMI_TAG_BAD_HEX;
                    x.kind = 2;
                    x.src = v;
                    x.len = digits;
                }
                q++;
                break;
            }
            case 'B': {
                if (v + 5 > end) return SMI_TAG_BAD_AUX;
                const uint8_t sub = bam[v];
                const uint32_t w = sub == 'c' || sub == 'C' ? 1 : sub == 's' || sub == 'S' ? 2 : sub == 'i' || sub == 'I' || sub == 'f' ? 4 : 0;
                if (!w) return SMI_TAG_BAD_AUX;
                q = v + 5 + (uint64_t)w * ld_u32(bam + v + 1);
                break;
            }
            default: return SMI_TAG_BAD_AUX;
        }
        if (q > end) return SMI_TAG_BAD_AUX;
        if (x.kind == 0) {
            x.src = p + 2;
            x.len = (uint32_t)(q - p - 2);
        }
        if (!put_field(f, n, x)) return SMI_TAG_TOO_MANY_ATTRS;
        p = q;
    }
    Field s = {};
    s.kind = 3;
    s.len = seq_len;
    s.key = (uint16_t)read_key;
    s.src = seq_start;
    if (!put_field(f, n, s)) return SMI_TAG_TOO_MANY_ATTRS;
    if (with_qv) {
        s.key = (uint16_t)qv_key;
        s.src = qual_start;
        s.len = qual_len;
        if (!put_field(f, n, s)) return SMI_TAG_TOO_MANY_ATTRS;
    }
    for (int i = 1; i < n; i++) {  // insertion sort by binary tag (keys are distinct)
        const Field x = f[i];
        int j = i - 1;
        while (j >= 0 && f[j].key > x.key) {
            f[j + 1] = f[j];
            j--;
        }
        f[j + 1] = x;
    }
    return 0;
}

template <bool WRITE>
__global__ __launch_bounds__(64 * kAsmWaves) void k_tag_asm(const uint8_t *__restrict__ bam, const smi_bam_record *__restrict__ recs, size_t n,
                                                             const int32_t *__restrict__ res, const uint8_t *__restrict__ text,
                                                             const uint64_t *__restrict__ seq_start, const uint32_t *__restrict__ seq_len,
                                                             const uint64_t *__restrict__ qual_start, const uint32_t *__restrict__ qual_len,
                                                             uint32_t read_key, uint32_t qv_key, int with_qv,
                                                             uint64_t *__restrict__ size, const uint64_t *__restrict__ off, uint8_t *__restrict__ out,
                                                             uint64_t out_cap, uint32_t *__restrict__ err) {
    __shared__ Field fields[kAsmWaves][kMaxFields];
    __shared__ int n_fields[kAsmWaves];
    __shared__ uint32_t bad[kAsmWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t i = blockIdx.x * (size_t)kAsmWaves + wv;
    if (i >= n) return;
    const int32_t fq = res[i];
    if (fq < 0) {
        if (!WRITE && lane == 0) size[i] = 0;  // dropped
        return;
    }
    const smi_bam_record rec = recs[i];
    Field *f = fields[wv];
    if (lane == 0) {
        int nf = 0;
        uint32_t b = parse_fields(bam, rec, text, seq_start[fq], qual_start[fq], seq_len[fq], qual_len[fq], read_key, qv_key, with_qv != 0, f, nf);
        uint64_t o = rec.aux_off - rec.rec_off;  // block_size word + fixed part + name + CIGAR + sequence + qualities
        for (int j = 0; j < nf; j++) {
            f[j].out = o;
            o += field_bytes(f[j]);
        }
        if (!WRITE) {
            size[i] = b ? 0 : o;
            if (b) atomicOr(err, b);
        } else if (!b && off[i] + o > out_cap) {
            b = SMI_TAG_OVERFLOW;  // (cannot happen with the sizes of the SIZE pass; never written past the buffer)
            atomicOr(err, b);
        }
        n_fields[wv] = nf;
        bad[wv] = b;
    }
    if (!WRITE) return;
    wave_sync();
    if (bad[wv]) return;
    const int nf = n_fields[wv];
    uint8_t *dst = out + off[i];
    const uint64_t fixed = rec.aux_off - rec.rec_off - 4;
    const uint64_t total = nf ? f[nf - 1].out + field_bytes(f[nf - 1]) : fixed + 4;
    if (lane == 0) {
        const uint32_t bs = (uint32_t)(total - 4);
        dst[0] = (uint8_t)bs;
        dst[1] = (uint8_t)(bs >> 8);
        dst[2] = (uint8_t)(bs >> 16);
        dst[3] = (uint8_t)(bs >> 24);
    }
    for (uint64_t k = lane; k < fixed; k += 64) dst[4 + k] = bam[rec.rec_off + 4 + k];
    for (int j = 0; j < nf; j++) {
        const Field x = f[j];
        uint8_t *d = dst + x.out;
        if (lane == 0) {
            d[0] = (uint8_t)x.key;
            d[1] = (uint8_t)(x.key >> 8);
        }
        switch (x.kind) {
            case 0:
                for (uint32_t k = lane; k < x.len; k += 64) d[2 + k] = bam[x.src + k];
                break;
            case 1:
                if (lane == 0) {
                    d[2] = x.type;
                    const uint32_t w = x.type == 'c' || x.type == 'C' ? 1 : x.type == 's' || x.type == 'S' ? 2 : 4;
                    const uint64_t u = (uint64_t)x.ival;
                    for (uint32_t k = 0; k < w; k++) d[3 + k] = (uint8_t)(u >> (8 * k));
                }
                break;
            case 2: {
                const uint32_t nb = x.len / 2;
                if (lane == 0) {
                    d[2] = 'B';
                    d[3] = 'c';
                    d[4] = (uint8_t)nb;
                    d[5] = (uint8_t)(nb >> 8);
                    d[6] = (uint8_t)(nb >> 16);
                    d[7] = (uint8_t)(nb >> 24);
                }
                for (uint32_t k = lane; k < nb; k += 64)
                    d[8 + k] = (uint8_t)(hex_val(bam[x.src + 2 * k]) << 4 | hex_val(bam[x.src + 2 * k + 1]));
                break;
            }
            default:
                if (lane == 0) {
                    d[2] = 'Z';
                    d[3 + x.len] = 0;
                }
                for (uint32_t k = lane; k < x.len; k += 64) d[3 + k] = text[x.src + k];
                break;
        }
    }
}

unsigned blocks_for(size_t n, unsigned per) { return (unsigned)std::max<size_t>(1, (n + per - 1) / per); }

}  // namespace

// K-TAG-ASM for records already on the device (smi_internal.h)
int tag_assemble_z2(hipStream_t s, const uint8_t *d_bam, const smi_bam_record *d_recs, size_t n, const int32_t *d_entry, const uint8_t *d_text,
                    const uint64_t *d_a_start, const uint32_t *d_a_len, const uint64_t *d_b_start, const uint32_t *d_b_len, const char *tag_a,
                    const char *tag_b, std::vector<uint8_t> &out, float *ms) {
    out.clear();
    if (!n) return SMI_OK;
    const uint32_t ka = (uint32_t)(uint8_t)tag_a[1] << 8 | (uint8_t)tag_a[0], kb = (uint32_t)(uint8_t)tag_b[1] << 8 | (uint8_t)tag_b[0];
    uint64_t *d_size = nullptr, *d_off = nullptr;
    uint32_t *d_err = nullptr;
    void *d_cub = nullptr;
    uint8_t *d_out = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = SMI_OK;
    auto fin = [&](int r) {
        for (void *p : {(void *)d_size, (void *)d_off, (void *)d_err, d_cub, (void *)d_out})
            if (p) (void)hipFree(p);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        return r;
    };
#define SMI_Z2(call)                                          \
    do {                                                      \
        hipError_t e__ = (call);                              \
        if (e__ != hipSuccess) return fin(hip_fail(e__, #call)); \
    } while (0)
    size_t cub = 0;
    SMI_Z2(hipcub::DeviceScan::ExclusiveSum(nullptr, cub, (uint64_t *)nullptr, (uint64_t *)nullptr, n + 1, s));
    SMI_Z2(hipMalloc((void **)&d_size, (n + 1) * 8));
    SMI_Z2(hipMalloc((void **)&d_off, (n + 1) * 8));
    SMI_Z2(hipMalloc((void **)&d_err, 4));
    SMI_Z2(hipMalloc(&d_cub, std::max<size_t>(cub, 1)));
    SMI_Z2(hipEventCreate(&e0));
    SMI_Z2(hipEventCreate(&e1));
    SMI_Z2(hipMemsetAsync(d_err, 0, 4, s));
    SMI_Z2(hipMemsetAsync(d_size + n, 0, 8, s));
    SMI_Z2(hipEventRecord(e0, s));
    hipLaunchKernelGGL(k_tag_asm<false>, dim3(blocks_for(n, kAsmWaves)), dim3(64 * kAsmWaves), 0, s, d_bam, d_recs, n, d_entry, d_text, d_a_start,
                       d_a_len, d_b_start, d_b_len, ka, kb, 1, d_size, (const uint64_t *)nullptr, (uint8_t *)nullptr, (uint64_t)0, d_err);
    SMI_Z2(hipGetLastError());
    SMI_Z2(hipcub::DeviceScan::ExclusiveSum(d_cub, cub, d_size, d_off, n + 1, s));
    uint64_t total = 0;
    uint32_t err = 0;
    SMI_Z2(hipMemcpyAsync(&total, d_off + n, 8, hipMemcpyDeviceToHost, s));
    SMI_Z2(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, s));
    SMI_Z2(hipStreamSynchronize(s));
    if (err) {
        set_error(std::string("a record's attributes cannot be rewritten:") + (err & SMI_TAG_BAD_AUX ? " malformed or unknown attribute type;" : "") +
                  (err & SMI_TAG_BAD_HEX ? " H attribute that is not hex;" : "") +
                  (err & SMI_TAG_TOO_MANY_ATTRS ? " more than " + std::to_string(kMaxFields) + " attributes;" : std::string()));
        return fin(SMI_ERR_INVALID);
    }
    SMI_Z2(hipMalloc((void **)&d_out, std::max<uint64_t>(total, 1)));
    hipLaunchKernelGGL(k_tag_asm<true>, dim3(blocks_for(n, kAsmWaves)), dim3(64 * kAsmWaves), 0, s, d_bam, d_recs, n, d_entry, d_text, d_a_start,
                       d_a_len, d_b_start, d_b_len, ka, kb, 1, (uint64_t *)nullptr, (const uint64_t *)d_off, d_out, (uint64_t)total, d_err);
    SMI_Z2(hipGetLastError());
    SMI_Z2(hipEventRecord(e1, s));
    out.resize(total);
    SMI_Z2(hipMemcpyAsync(out.data(), d_out, total, hipMemcpyDeviceToHost, s));
    SMI_Z2(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, s));
    SMI_Z2(hipStreamSynchronize(s));
#undef SMI_Z2
    if (ms) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, e0, e1) == hipSuccess) *ms += t;
    }
    if (err) {
        set_error("the output buffer of the device was too small for a record (internal error)");
        rc = SMI_ERR_INVALID;
    }
    return fin(rc);
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
    uint64_t *d_size = nullptr, *d_off = nullptr;
    size_t rec_cap = 0;
    void *d_cub = nullptr;
    size_t cub_cap = 0;
    uint8_t *d_out = nullptr;
    size_t out_cap = 0;
    uint32_t *d_err = nullptr;
    std::vector<int32_t> res;
    // the segment the last call sized and did not write (out too small / NULL): the next call with the same arguments writes it
    const uint8_t *last_bam = nullptr;
    const smi_bam_record *last_recs = nullptr;
    size_t last_n_bam = 0;
    int32_t last_n = -1;
    uint64_t last_total = 0;
    hipEvent_t ev[6] = {};
    float ms[SMI_TAGBAM_STAGES] = {};
};

namespace {

void tagbam_release(smi_tagbam *h) {
    void *bufs[] = {h->d_text, h->d_line_start, h->d_name_start, h->d_seq_start, h->d_qual_start, h->d_offsets, h->d_name_len, h->d_seq_len,
                    h->d_key_len, h->d_table, h->d_bam, h->d_recs, h->d_res, h->d_size, h->d_off, h->d_cub, h->d_out, h->d_err};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
}

int valid_tag(const char *t) { return t[0] > ' ' && t[0] <= '~' && t[1] > ' ' && t[1] <= '~' && t[2] == 0; }

uint32_t tag_key(const char *t) { return (uint32_t)(uint8_t)t[1] << 8 | (uint8_t)t[0]; }

template <class T>
int grow(T **p, size_t &cap, size_t want) {  // device buffer of at least `want` elements (contents not kept)
    if (want <= cap && *p) return SMI_OK;
    if (*p) SMI_HIP(hipFree(*p));
    *p = nullptr;
    cap = 0;
    const size_t n = std::max<size_t>(want + want / 4, 1024);
    SMI_HIP(hipMalloc((void **)p, n * sizeof(T)));
    cap = n;
    return SMI_OK;
}

float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
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
    TAG_HIP(hipMalloc(&h->d_err, 4));
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
        size_t cub = 0;
        SMI_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, cub, (uint64_t *)nullptr, (uint64_t *)nullptr, n + 1, s));
        if (int rc = grow(&h->d_bam, h->bam_cap, n_bam + 1)) return rc;
        size_t c0 = h->rec_cap, c1 = h->rec_cap, c2 = h->rec_cap, c3 = h->rec_cap;
        if ((size_t)n + 1 > h->rec_cap || !h->d_recs) {
            if (int rc = grow(&h->d_recs, c0, (size_t)n + 1)) return rc;
            if (int rc = grow(&h->d_res, c1, (size_t)n + 1)) return rc;
            if (int rc = grow(&h->d_size, c2, (size_t)n + 1)) return rc;
            if (int rc = grow(&h->d_off, c3, (size_t)n + 1)) return rc;
            h->rec_cap = std::min(std::min(c0, c1), std::min(c2, c3));
        }
        if (int rc = grow((uint8_t **)&h->d_cub, h->cub_cap, cub)) return rc;
        if (n_bam) SMI_HIP(hipMemcpyAsync(h->d_bam, bam, n_bam, hipMemcpyHostToDevice, s));
        if (n) SMI_HIP(hipMemcpyAsync(h->d_recs, recs, (size_t)n * sizeof(smi_bam_record), hipMemcpyHostToDevice, s));
        SMI_HIP(hipMemsetAsync(h->d_err, 0, 4, s));
        SMI_HIP(hipMemsetAsync(h->d_size + n, 0, 8, s));
        const uint32_t rk = tag_key(h->cfg.read_tag), qk = tag_key(h->cfg.qv_tag);
        SMI_HIP(hipEventRecord(h->ev[2], s));
        if (n)
            hipLaunchKernelGGL(k_tag_probe, dim3(blocks_for(n, 256)), dim3(256), 0, s, (const uint8_t *)h->d_bam, (const smi_bam_record *)h->d_recs,
                               (size_t)n, (const uint8_t *)h->d_text, (const uint64_t *)h->d_name_start, (const uint32_t *)h->d_key_len,
                               (const uint64_t *)h->d_table, h->mask, h->hash_mask, h->d_res);
        SMI_HIP(hipGetLastError());
        SMI_HIP(hipEventRecord(h->ev[3], s));
        if (n)
            hipLaunchKernelGGL(k_tag_asm<false>, dim3(blocks_for(n, kAsmWaves)), dim3(64 * kAsmWaves), 0, s, (const uint8_t *)h->d_bam,
                               (const smi_bam_record *)h->d_recs, (size_t)n, (const int32_t *)h->d_res, (const uint8_t *)h->d_text,
                               (const uint64_t *)h->d_seq_start, (const uint32_t *)h->d_seq_len, (const uint64_t *)h->d_qual_start,
                               (const uint32_t *)h->d_seq_len, rk, qk,
                               h->cfg.with_qv, h->d_size, (const uint64_t *)nullptr, (uint8_t *)nullptr, (uint64_t)0, h->d_err);
        SMI_HIP(hipGetLastError());
        SMI_HIP(hipcub::DeviceScan::ExclusiveSum(h->d_cub, cub, h->d_size, h->d_off, n + 1, s));
        SMI_HIP(hipEventRecord(h->ev[4], s));
        h->res.resize((size_t)n + 1);
        uint32_t err = 0;
        if (n) SMI_HIP(hipMemcpyAsync(h->res.data(), h->d_res, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipMemcpyAsync(&total, h->d_off + n, 8, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipMemcpyAsync(&err, h->d_err, 4, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipStreamSynchronize(s));
        h->ms[2] = elapsed(h->ev[2], h->ev[3]);
        h->ms[3] = elapsed(h->ev[3], h->ev[4]);
        if (err) {
            set_error(std::string("smi_tagbam_segment: a record's attributes cannot be rewritten:") +
                      (err & SMI_TAG_BAD_AUX ? " malformed or unknown attribute type;" : "") + (err & SMI_TAG_BAD_HEX ? " H attribute that is not hex;" : "") +
                      (err & SMI_TAG_TOO_MANY_ATTRS ? " more than " + std::to_string(kMaxFields) + " attributes;" : std::string()));
            return SMI_ERR_INVALID;
        }
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
    if (int rc = grow(&h->d_out, h->out_cap, total)) return rc;
    SMI_HIP(hipEventRecord(h->ev[4], s));
    hipLaunchKernelGGL(k_tag_asm<true>, dim3(blocks_for(n, kAsmWaves)), dim3(64 * kAsmWaves), 0, s, (const uint8_t *)h->d_bam,
                       (const smi_bam_record *)h->d_recs, (size_t)n, (const int32_t *)h->d_res, (const uint8_t *)h->d_text,
                       (const uint64_t *)h->d_seq_start, (const uint32_t *)h->d_seq_len, (const uint64_t *)h->d_qual_start, (const uint32_t *)h->d_seq_len,
                       tag_key(h->cfg.read_tag),
                       tag_key(h->cfg.qv_tag), h->cfg.with_qv, (uint64_t *)nullptr, (const uint64_t *)h->d_off, h->d_out, (uint64_t)h->out_cap, h->d_err);
    SMI_HIP(hipGetLastError());
    SMI_HIP(hipEventRecord(h->ev[5], s));
    uint32_t err = 0;
    SMI_HIP(hipMemcpyAsync(&err, h->d_err, 4, hipMemcpyDeviceToHost, s));
    SMI_HIP(hipMemcpyAsync(out, h->d_out, total, hipMemcpyDeviceToHost, s));
    SMI_HIP(hipStreamSynchronize(s));
    h->ms[4] = elapsed(h->ev[4], h->ev[5]);
    if (err) {
        set_error("smi_tagbam_segment: the output buffer of the device was too small for a record (internal error)");
        return SMI_ERR_INVALID;
    }
    return SMI_OK;
}
