// smi_auxedit.h -- the attribute rewrite of BAM records on the device, shared by K-TAG-ASM (`tagbamwithread` and IsoformMatrix's ISOBAM,
// smi_tagbam.hip) and K-EDIT (`AddBamMoleculeTags` / `AddGeneNameTag`, smi_moltag.hip).
//
// The attribute list is what htsjdk writes after setAttribute (BinaryTagCodec.readTags L271-305 + SAMBinaryTagAndValue.insert L207-228,
// pinned by tests/golden/ref_exec_auxorder.json): ordered by binary tag, a repeated tag keeping its last value, integers in the smallest
// type (getIntegerType L153-180), H read back as a byte array (B:c).
//
// k_aux_rewrite<WRITE, Source>: one wavefront per record, four per block.  SIZE (lane 0 parses the attributes and sizes the record) and
// WRITE (lane 0 parses into LDS; the wavefront copies the fixed part, the attributes and the Z payloads into the output at the offset of
// the exclusive scan of the sizes).  What differs between the programs is the Source, passed by value as a kernel argument:
//   bool keeps(size_t i) const              is record i written at all?  Asked BEFORE its attributes are read: a dropped record is never parsed
//   Tail tail(size_t i) const               what follows the walk of record i, fetched before the walk starts;
//   uint32_t Tail::put(Field *f, int &n)    ... applied after it as put_field / remove_field calls in order -> SMI_TAG_* error bits
//   const uint8_t *payload() const          the byte array the kind-3 (Z) payloads are copied from
// AuxRewriter is the host side of the sequence: SIZE launch, hipcub exclusive scan, WRITE launch, with the buffers they need.
// (ld_u32, st_u32 and the hipcub scratch are smi_device.h's.)
#pragma once
#include <algorithm>
#include <functional>
#include <string>

#include "smi_device.h"
#include "smi_internal.h"

namespace smi {

constexpr int kMaxFields = SMI_TAGBAM_MAX_ATTRS;
constexpr int kAuxWaves = 4;  // waves per block of k_aux_rewrite

// one attribute of the written record
struct Field {
    uint16_t key;    // binary tag: second char << 8 | first char (SAMTag.makeBinaryTag L124-127)
    uint8_t kind;    // 0 verbatim (src: type byte .. end), 1 integer (ival), 2 H -> B:c (src: the hex digits), 3 Z from the source's payload bytes
    uint8_t type;    // output type of an integer
    uint32_t len;    // kind 0: bytes behind the tag; 2: hex digits; 3: payload bytes
    uint64_t src;    // kind 0 / 2: offset in the BAM stream; 3: offset in the payload bytes
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

// insert or replace (a repeated tag keeps its last value); false: more than kMaxFields attributes
static __device__ bool put_field(Field *f, int &n, const Field &x) {
    for (int j = 0; j < n; j++)
        if (f[j].key == x.key) {
            f[j] = x;
            return true;
        }
    if (n >= kMaxFields) return false;
    f[n++] = x;
    return true;
}
// setAttribute(tag, null): an absent tag is a no-op
__device__ __forceinline__ void remove_field(Field *f, int &n, uint16_t key) {
    for (int j = 0; j < n; j++)
        if (f[j].key == key) {
            for (int m = j + 1; m < n; m++) f[m - 1] = f[m];
            n--;
            return;
        }
}

// lane 0: the attribute list of record rec as written (its own attributes, then what `tail` puts), in f[0 .. n), sorted by binary tag;
// returns SMI_TAG_* error bits (0 = fine).  The walk decodes each value where it steps over it, so it carries the size rule of lr::aux_size
// (smi_longread.h) itself: stepping with that function and decoding after it cost K-TAG-ASM's WRITE pass 2.4 % (profiles/device_layer_compare.md);
// the damaged lists of tests/auxcases.py go through both.
template <class Tail>
static __device__ uint32_t parse_fields(const uint8_t *__restrict__ bam, const smi_bam_record &rec, const Tail &tail, Field *f, int &n) {
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
    if (const uint32_t b = tail.put(f, n)) return b;
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

template <bool WRITE, class Source>
__global__ __launch_bounds__(64 * kAuxWaves) void k_aux_rewrite(const uint8_t *__restrict__ bam, const smi_bam_record *__restrict__ recs, size_t n,
                                                                 const Source src, uint64_t *__restrict__ size, const uint64_t *__restrict__ off,
                                                                 uint8_t *__restrict__ out, uint64_t out_cap, uint32_t *__restrict__ err) {
    __shared__ Field fields[kAuxWaves][kMaxFields];
    __shared__ int n_fields[kAuxWaves];
    __shared__ uint32_t bad[kAuxWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t i = blockIdx.x * (size_t)kAuxWaves + wv;
    if (i >= n) return;
    if (!src.keeps(i)) {
        if (!WRITE && lane == 0) size[i] = 0;  // dropped
        return;
    }
    const smi_bam_record rec = recs[i];
    Field *f = fields[wv];
    if (lane == 0) {
        int nf = 0;
        uint32_t b = parse_fields(bam, rec, src.tail(i), f, nf);
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
    const uint8_t *__restrict__ payload = src.payload();
    const int nf = n_fields[wv];
    uint8_t *dst = out + off[i];
    const uint64_t fixed = rec.aux_off - rec.rec_off - 4;
    const uint64_t total = nf ? f[nf - 1].out + field_bytes(f[nf - 1]) : fixed + 4;
    if (lane == 0) st_u32(dst, (uint32_t)(total - 4));
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
                    st_u32(d + 4, nb);
                }
                for (uint32_t k = lane; k < nb; k += 64)
                    d[8 + k] = (uint8_t)(hex_val(bam[x.src + 2 * k]) << 4 | hex_val(bam[x.src + 2 * k + 1]));
                break;
            }
            default:
                if (lane == 0) {
                    d[2] = 'Z';
                    d[3 + x.len] = 0;  // a payload of length 0 is the empty string
                }
                for (uint32_t k = lane; k < x.len; k += 64) d[3 + k] = payload[x.src + k];
                break;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
inline unsigned blocks_for(size_t n, unsigned per) { return (unsigned)std::max<size_t>(1, (n + per - 1) / per); }
inline uint32_t tag_key(const char *t) { return (uint32_t)(uint8_t)t[1] << 8 | (uint8_t)t[0]; }

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

inline float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}

// the text for the SMI_TAG_* bits of a rewrite, behind the caller's own prefix
inline std::string aux_error_text(uint32_t err) {
    if (err & SMI_TAG_OVERFLOW) return "the output buffer of the device was too small for a record (internal error)";
    return std::string("a record's attributes cannot be rewritten:") + (err & SMI_TAG_BAD_AUX ? " malformed or unknown attribute type;" : "") +
           (err & SMI_TAG_BAD_HEX ? " H attribute that is not hex;" : "") +
           (err & SMI_TAG_TOO_MANY_ATTRS ? " more than " + std::to_string(kMaxFields) + " attributes;" : std::string());
}

// SIZE launch + exclusive scan, then WRITE launch, over n records on the device; the sizes, offsets, scan scratch, output and error word
// are its own (grow-only).  size() and write() are two calls because the callers hand the total out between them (sizes first; the next
// call with the same arguments writes).  Both wait for the stream.  A record that cannot be rewritten ends either call with SMI_ERR_INVALID,
// the SMI_TAG_* bits in `err` and the error text set: `who` (the caller's prefix) + aux_error_text(err).
struct AuxRewriter {
    uint64_t *d_size = nullptr, *d_off = nullptr;
    size_t size_cap = 0, off_cap = 0;
    Scratch cub{"the attribute rewrite"};
    uint8_t *d_out = nullptr;
    size_t out_cap = 0;
    uint32_t *d_err = nullptr, err = 0;  // err: the bits of the last size() / write()
    hipEvent_t ev[2] = {};

    AuxRewriter() = default;
    AuxRewriter(const AuxRewriter &) = delete;
    ~AuxRewriter() {  // (on the device of the buffers: the owners set it before they release)
        for (void *p : {(void *)d_size, (void *)d_off, (void *)d_out, (void *)d_err})
            if (p) (void)hipFree(p);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }

    // *total: bytes of the records src keeps; *ms: device time of SIZE + scan.  before_wait (may be empty) is called once everything is
    // enqueued: what the caller wants read back on the same wait, so that the host stays ahead of the device up to that point
    template <class Source>
    int size(const char *who, hipStream_t s, const uint8_t *d_bam, const smi_bam_record *d_recs, size_t n, const Source &src, uint64_t *total,
             float *ms, const std::function<hipError_t()> &before_wait = nullptr) {
        *total = 0;
        err = 0;
        if (int rc = grow(&d_size, size_cap, n + 1)) return rc;
        if (int rc = grow(&d_off, off_cap, n + 1)) return rc;
        const auto scan = [&](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, d_size, d_off, n + 1, s); };
        if (int rc = reserve(cub, scan)) return rc;
        if (!d_err) SMI_HIP(hipMalloc((void **)&d_err, 4));
        for (hipEvent_t &e : ev)
            if (!e) SMI_HIP(hipEventCreate(&e));
        SMI_HIP(hipMemsetAsync(d_err, 0, 4, s));
        SMI_HIP(hipMemsetAsync(d_size + n, 0, 8, s));
        SMI_HIP(hipEventRecord(ev[0], s));
        if (n)
            hipLaunchKernelGGL((k_aux_rewrite<false, Source>), dim3(blocks_for(n, kAuxWaves)), dim3(64 * kAuxWaves), 0, s, d_bam, d_recs, n, src, d_size,
                               (const uint64_t *)nullptr, (uint8_t *)nullptr, (uint64_t)0, d_err);
        SMI_HIP(hipGetLastError());
        if (int rc = run_reserved(cub, scan)) return rc;
        SMI_HIP(hipEventRecord(ev[1], s));
        SMI_HIP(hipMemcpyAsync(total, d_off + n, 8, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, s));
        if (before_wait) SMI_HIP(before_wait());
        SMI_HIP(hipStreamSynchronize(s));
        *ms = elapsed(ev[0], ev[1]);
        return finish(who);
    }

    // the records size() measured (same arguments, total > 0) -> out[0 .. total) on the host; *ms: device time of WRITE
    template <class Source>
    int write(const char *who, hipStream_t s, const uint8_t *d_bam, const smi_bam_record *d_recs, size_t n, const Source &src, uint64_t total,
              uint8_t *out, float *ms) {
        if (int rc = grow(&d_out, out_cap, total)) return rc;
        SMI_HIP(hipEventRecord(ev[0], s));
        hipLaunchKernelGGL((k_aux_rewrite<true, Source>), dim3(blocks_for(n, kAuxWaves)), dim3(64 * kAuxWaves), 0, s, d_bam, d_recs, n, src,
                           (uint64_t *)nullptr, (const uint64_t *)d_off, d_out, (uint64_t)out_cap, d_err);
        SMI_HIP(hipGetLastError());
        SMI_HIP(hipEventRecord(ev[1], s));
        SMI_HIP(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipStreamSynchronize(s));
        *ms = elapsed(ev[0], ev[1]);
        return finish(who);
    }

    int finish(const char *who) const {
        if (!err) return SMI_OK;
        set_error(who + aux_error_text(err));
        return SMI_ERR_INVALID;
    }
};

}  // namespace smi
