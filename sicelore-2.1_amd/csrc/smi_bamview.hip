// smi_bamview.hip -- `BamView`: the records of a BAM that pass the flag and quality filters and overlap one of the regions, in file order,
// in the place of `samtools view -b in.bam [region ...]`.  The definition is DESIGN.md section 8o (tests/viewmodel.py restates it): the
// extent of a record is 8l's (pos, pos + the M D N = X lengths of the stored CIGAR; one base where that sum is 0, where there is no CIGAR
// and where flag 0x4 is set), a record overlaps (ref, b, e) when ref_id == ref, beg < e and end > b, compared in 64 bits.
//
// The caller hands in inflated bytes with their record index (smi_bamview_add_segment): the whole stream in segments, or the bytes under
// the ranges an index gave for the regions.  The host has merged the regions of every reference into disjoint, sorted intervals
// (smi_bamview_create).  Per segment
//   K-VIEW-TEST    kCopyLanes lanes per record sum the CIGAR's reference length 64 bytes at a time (sub-wave shuffle reduction, as
//                  K-BAI-REC); lane 0 of the group applies the filters and finds, by binary search in the reference's slice of the interval
//                  array, the first interval that ends behind the record's begin: the record is kept iff that interval begins in front of
//                  its end.  It writes the record's size (0 where it is dropped) and a keep flag; a ref_id outside the header stops the run
//                  (atomicMin of the record number)
//   hipcub         exclusive sum of the n + 1 sizes: every kept record's offset in the output and the total; a sum of the keep flags: how
//                  many records stay
// and (smi_bamview_convert)
//   K-VIEW-GATHER  kCopyLanes lanes per kept record copy it, with its block_size word, to its offset (copy_record, smi_device.h); the
//                  groups of dropped records return at once
// and the library's BGZF deflater (smi_bgzf_deflate_device) on the output buffer.  Integer work only.  Every load lies inside a record of
// the uploaded bytes (the host checks the index entries before they go up), every store inside the record's place in the output.
#include <chrono>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "smi_device.h"
#include "smi_handle.h"
#include "smi_internal.h"

#define VIEW_HD __host__ __device__ __forceinline__

namespace smi {
namespace {

constexpr int kViewBlock = 256;
constexpr int kViewLanes = kCopyLanes;  // lanes per record of both kernels (why 16)
constexpr int kViewRecs = kViewBlock / kViewLanes;
constexpr unsigned long long kNoRecord = ~0ull;
enum { W_STOP = 0, W_KEPT, W_COUNT };

struct Filters {
    uint32_t require, exclude, min_mapq, has_regions;
    const uint32_t *ref_begin;  // [n_ref + 1] into ibeg / iend
    const long long *ibeg, *iend;  // disjoint, ascending inside a reference; half-open
};

VIEW_HD bool on_reference(uint32_t word) { return (0x18Du >> (word & 15u)) & 1u; }  // M D N = X

// the filters and the region test of one record; ref < n_ref.  sum: the reference length of its stored CIGAR
VIEW_HD bool view_keep(const Filters &f, uint32_t flag, uint32_t mapq, int32_t ref, int32_t pos, uint32_t n_cigar, unsigned long long sum) {
    if ((flag & f.require) != f.require || (flag & f.exclude) || mapq < f.min_mapq) return false;
    if (!f.has_regions) return true;
    if (ref < 0) return false;
    const long long beg = pos, end = beg + (long long)((flag & 4u) || !n_cigar || !sum ? 1ull : sum);
    const uint32_t last = f.ref_begin[ref + 1];
    uint32_t lo = f.ref_begin[ref], hi = last;  // the first interval with iend > beg
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (f.iend[mid] > beg) hi = mid;
        else lo = mid + 1;
    }
    return lo < last && f.ibeg[lo] < end;
}

// K-VIEW-TEST: bam holds the stream's bytes from `first` on; size[i] = the bytes record i takes in the output, keep[i] = 1 where it stays
__global__ __launch_bounds__(kViewBlock) void k_view_test(const uint8_t *__restrict__ bam, const smi_bam_record *__restrict__ recs, uint32_t n, int32_t n_ref,
                                                          uint64_t first, Filters f, uint64_t *__restrict__ size, uint8_t *__restrict__ keep,
                                                          unsigned long long *__restrict__ words) {
    const uint32_t i = blockIdx.x * kViewRecs + (threadIdx.x / kViewLanes), sub = threadIdx.x % kViewLanes;
    const bool valid = i < n;
    unsigned long long sum = 0;
    uint32_t n_cigar = 0, rec_len = 0, flag = 0, mapq = 0;
    int32_t ref = -1, pos = 0;
    if (valid) {
        const smi_bam_record *r = recs + i;
        const uint8_t *__restrict__ cigar = bam + (r->cigar_off - first);
        n_cigar = r->n_cigar;
        rec_len = r->rec_len;
        flag = r->flag;
        mapq = r->mapq;
        ref = r->ref_id;
        pos = r->pos;
        if (f.has_regions)
            for (uint32_t k = sub; k < n_cigar; k += kViewLanes) {
                const uint32_t w = ld_u32(cigar + 4ull * k);
                if (on_reference(w)) sum += w >> 4;
            }
    }
#pragma unroll
    for (int m = kViewLanes / 2; m; m >>= 1) sum += __shfl_xor(sum, m, kViewLanes);
    if (!valid || sub) return;
    bool kept = false;
    if (ref >= n_ref) atomicMin(words + W_STOP, (unsigned long long)i);
    else kept = view_keep(f, flag, mapq, ref, pos, n_cigar, sum);
    size[i] = kept ? rec_len : 0u;
    keep[i] = kept;
}

// K-VIEW-GATHER: kept record i to dst + off[i]; dst is aligned to 256 bytes
__global__ __launch_bounds__(kViewBlock) void k_view_gather(const uint8_t *__restrict__ bam, const smi_bam_record *__restrict__ recs, uint32_t n, uint64_t first,
                                                            const uint8_t *__restrict__ keep, const uint64_t *__restrict__ off, uint8_t *__restrict__ dst) {
    const uint32_t i = blockIdx.x * kViewRecs + (threadIdx.x / kViewLanes), sub = threadIdx.x % kViewLanes;
    if (i >= n || !keep[i]) return;
    copy_record<16>(bam + (recs[i].rec_off - first), recs[i].rec_len, off[i], dst, sub);
}

struct AsCount {  // a keep flag as a number to sum
    __host__ __device__ unsigned long long operator()(uint8_t k) const { return k; }
};

template <class T>
int view_grow(T **p, size_t &cap, size_t want) {
    if (want <= cap && *p) return SMI_OK;
    const size_t n = std::max<size_t>(want + want / 4, 1024);
    if (*p) SMI_HIP(hipFree(*p));
    *p = nullptr;
    cap = 0;
    if (hipMalloc((void **)p, n * sizeof(T)) != hipSuccess) {
        *p = nullptr;
        set_error("BamView: device allocation of " + std::to_string(n * sizeof(T)) + " bytes failed");
        return SMI_ERR_HIP;
    }
    cap = n;
    return SMI_OK;
}

inline unsigned view_grid(size_t n) { return (unsigned)std::max<size_t>(1, (n + kViewRecs - 1) / kViewRecs); }

}  // namespace
}  // namespace smi

using namespace smi;

struct smi_bamview {
    smi_ctx *ctx = nullptr;
    int32_t n_ref = 0;
    Filters f = {};  // its pointers: the device's arrays
    std::vector<uint32_t> ref_begin;  // the host's copy (smi_bamview_host_loop)
    std::vector<long long> ibeg, iend;
    uint32_t *d_ref_begin = nullptr;
    long long *d_ibeg = nullptr, *d_iend = nullptr;
    // one segment (grow-only)
    uint8_t *d_bam = nullptr, *d_keep = nullptr, *d_out = nullptr;
    smi_bam_record *d_recs = nullptr;
    uint64_t *d_off = nullptr;
    size_t bam_cap = 0, keep_cap = 0, out_cap = 0, recs_cap = 0, off_cap = 0;
    unsigned long long *d_words = nullptr;
    Scratch cub{"BamView"};
    size_t n_bam = 0, n = 0, n_out = 0, n_kept = 0;  // of the segment taken last
    uint64_t first = 0;
    bool sized = false, written = false, failed = false;
    Events ev;
    int64_t counts[SMI_BAMVIEW_N_COUNT] = {};
    float ms[SMI_BAMVIEW_N_STAGE] = {};
    std::string error_read;
    int64_t error_record = -1;
};

namespace {

void view_release(smi_bamview *h) {
    void *bufs[] = {h->d_ref_begin, h->d_ibeg, h->d_iend, h->d_bam, h->d_keep, h->d_out, h->d_recs, h->d_off, h->d_words};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    delete h;
}

template <class T>
int view_put(T **d, const std::vector<T> &v) {
    SMI_HIP(hipMalloc((void **)d, std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (!v.empty()) SMI_HIP(hipMemcpy(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return SMI_OK;
}

}  // namespace

extern "C" int smi_bamview_create(smi_ctx *ctx, int32_t n_ref, uint32_t require, uint32_t exclude, uint32_t min_mapq, const int32_t *region_ref,
                                  const int64_t *region_beg, const int64_t *region_end, size_t n_regions, smi_bamview **out) {
    if (!ctx || !out || n_ref < 0 || (n_regions && (!region_ref || !region_beg || !region_end)) || n_regions > (size_t)INT32_MAX) {
        set_error("smi_bamview_create: bad argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    // disjoint intervals in ascending order, reference by reference: the binary search of K-VIEW-TEST rests on it
    for (size_t k = 0; k < n_regions; k++) {
        const bool ok = region_ref[k] >= 0 && region_ref[k] < n_ref && region_beg[k] >= 0 && region_end[k] > region_beg[k] &&
                        (!k || region_ref[k] > region_ref[k - 1] || (region_ref[k] == region_ref[k - 1] && region_beg[k] > region_end[k - 1]));
        if (!ok) {
            set_error("smi_bamview_create: region " + std::to_string(k) + " is empty, outside the references, or not merged and sorted");
            return SMI_ERR_INVALID;
        }
    }
    SMI_HIP(hipSetDevice(ctx->device));
    smi_bamview *h = new smi_bamview();
    h->ctx = ctx;
    h->n_ref = n_ref;
    h->ref_begin.assign((size_t)n_ref + 1, 0);
    for (size_t k = 0; k < n_regions; k++) {
        h->ref_begin[(size_t)region_ref[k] + 1]++;
        h->ibeg.push_back(region_beg[k]);
        h->iend.push_back(region_end[k]);
    }
    for (int32_t r = 0; r < n_ref; r++) h->ref_begin[(size_t)r + 1] += h->ref_begin[r];
    int rc = SMI_OK;
    if (n_regions) {
        rc = view_put(&h->d_ref_begin, h->ref_begin);
        if (!rc) rc = view_put(&h->d_ibeg, h->ibeg);
        if (!rc) rc = view_put(&h->d_iend, h->iend);
    }
    if (!rc && hipMalloc((void **)&h->d_words, W_COUNT * sizeof(unsigned long long)) != hipSuccess) rc = hip_fail(hipErrorOutOfMemory, "smi_bamview_create");
    if (rc) {
        view_release(h);
        return rc;
    }
    h->f = Filters{require, exclude, min_mapq, n_regions ? 1u : 0u, h->d_ref_begin, h->d_ibeg, h->d_iend};
    h->counts[SMI_BAMVIEW_REGIONS] = (int64_t)n_regions;
    *out = h;
    return SMI_OK;
}

extern "C" int smi_bamview_free(smi_bamview *h) {
    if (h) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        view_release(h);
    }
    return SMI_OK;
}

extern "C" int smi_bamview_counts(const smi_bamview *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_bamview_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof h->counts);
    return SMI_OK;
}

extern "C" int smi_bamview_stage_ms(const smi_bamview *h, float *ms) {
    if (!h || !ms) {
        set_error("smi_bamview_stage_ms: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(ms, h->ms, sizeof h->ms);
    return SMI_OK;
}

extern "C" int smi_bamview_error_read(const smi_bamview *h, char *name, size_t cap, int64_t *record) {
    if (!h || !record || (cap && !name)) {
        set_error("smi_bamview_error_read: null argument");
        return SMI_ERR_INVALID;
    }
    return handle::error_read(h->error_read, h->error_record, name, cap, record);
}

extern "C" int smi_bamview_add_segment(smi_bamview *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n, size_t *n_bgzf,
                                       size_t *n_record_bytes) {
    if (!h || n < 0 || !n_bgzf || !n_record_bytes || (n && (!bam || !recs))) {
        set_error("smi_bamview_add_segment: bad argument");
        return SMI_ERR_INVALID;
    }
    *n_bgzf = *n_record_bytes = 0;
    if (h->failed) {
        set_error("smi_bamview_add_segment: an earlier call failed");
        return SMI_ERR_STATE;
    }
    // every record inside the buffer, one behind the other, and its CIGAR inside the record: the kernels read nothing else
    for (int32_t i = 0; i < n; i++) {
        const smi_bam_record &r = recs[i];
        if (r.rec_len < 36 || r.rec_off > n_bam || r.rec_len > n_bam - r.rec_off || r.name_off < r.rec_off ||
            r.name_off + r.l_read_name > r.rec_off + r.rec_len || r.cigar_off < r.rec_off || r.cigar_off + 4ull * r.n_cigar > r.rec_off + r.rec_len ||
            (i && r.rec_off < recs[i - 1].rec_off + recs[i - 1].rec_len)) {
            set_error("smi_bamview_add_segment: record index entry " + std::to_string(i) + " points outside the BAM buffer");
            return SMI_ERR_INVALID;
        }
    }
    if (n >= INT32_MAX - 1) {  // hipcub counts in int
        set_error("BamView: more than 2^31 - 3 records in one segment: pass smaller segments");
        return SMI_ERR_INVALID;
    }
    h->sized = h->written = false;
    h->n_bam = h->n = h->n_out = h->n_kept = 0;
    std::memset(h->ms, 0, sizeof h->ms);
    if (!n) {
        h->sized = true;
        return smi_bgzf_deflate_device(h->ctx, h->d_out, 0, nullptr, 0, n_bgzf);
    }
    const size_t N = (size_t)n;
    const uint64_t first = recs[0].rec_off, last = recs[n - 1].rec_off + recs[n - 1].rec_len;
    const size_t bytes = (size_t)(last - first);
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    if (int rc = view_grow(&h->d_bam, h->bam_cap, bytes + 16)) return rc;
    if (int rc = view_grow(&h->d_recs, h->recs_cap, N)) return rc;
    if (int rc = view_grow(&h->d_keep, h->keep_cap, N)) return rc;
    if (int rc = view_grow(&h->d_off, h->off_cap, N + 1)) return rc;
    h->failed = true;  // until the segment is through
    SMI_HIP(hipMemcpyAsync(h->d_bam, bam + first, bytes, hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemcpyAsync(h->d_recs, recs, N * sizeof(smi_bam_record), hipMemcpyHostToDevice, s));
    const unsigned long long words0[W_COUNT] = {kNoRecord, 0ull};
    SMI_HIP(hipMemcpyAsync(h->d_words, words0, sizeof words0, hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemsetAsync(h->d_off + N, 0, 8, s));
    const auto offsets = [&](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, h->d_off, h->d_off, (int)(N + 1), s); };
    const hipcub::TransformInputIterator<unsigned long long, AsCount, const uint8_t *> flags(h->d_keep, AsCount());
    const auto kept = [&](void *p, size_t &t) { return hipcub::DeviceReduce::Sum(p, t, flags, h->d_words + W_KEPT, (int)N, s); };
    if (int rc = reserve(h->cub, offsets, kept)) return rc;
    if (int rc = h->ev.begin(s)) return rc;
    hipLaunchKernelGGL(k_view_test, dim3(view_grid(N)), dim3(kViewBlock), 0, s, (const uint8_t *)h->d_bam, (const smi_bam_record *)h->d_recs, (uint32_t)n, h->n_ref,
                       first, h->f, h->d_off, h->d_keep, h->d_words);
    SMI_HIP(hipGetLastError());
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMVIEW_MS_TEST])) return rc;
    if (int rc = h->ev.begin(s)) return rc;
    if (int rc = run_reserved(h->cub, offsets)) return rc;
    if (int rc = run_reserved(h->cub, kept)) return rc;
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMVIEW_MS_SCAN])) return rc;
    unsigned long long words[W_COUNT] = {kNoRecord, 0ull};
    uint64_t total = 0;
    SMI_HIP(hipMemcpyAsync(words, h->d_words, sizeof words, hipMemcpyDeviceToHost, s));
    SMI_HIP(hipMemcpyAsync(&total, h->d_off + N, 8, hipMemcpyDeviceToHost, s));
    SMI_HIP(hipStreamSynchronize(s));
    if (words[W_STOP] != kNoRecord) {
        const smi_bam_record &r = recs[words[W_STOP]];
        h->error_read.assign((const char *)bam + r.name_off, r.l_read_name ? r.l_read_name - 1u : 0u);
        h->error_record = h->counts[SMI_BAMVIEW_RECORDS] + (int64_t)words[W_STOP];
        set_error("read " + h->error_read + " (record " + std::to_string(h->error_record) + "): its ref_id is not one of the header's references");
        return 2;
    }
    if (total > bytes || words[W_KEPT] > N) {  // (cannot happen: the kept records are some of the segment's)
        set_error("BamView: the kept records exceed the segment");
        return SMI_ERR_STATE;
    }
    if (int rc = view_grow(&h->d_out, h->out_cap, (size_t)total + 16)) return rc;
    h->n_bam = bytes;
    h->n = N;
    h->first = first;
    h->n_out = (size_t)total;
    h->n_kept = (size_t)words[W_KEPT];
    h->sized = true;
    h->failed = false;
    *n_record_bytes = (size_t)total;
    return smi_bgzf_deflate_device(h->ctx, h->d_out, (size_t)total, nullptr, 0, n_bgzf);
}

extern "C" int smi_bamview_convert(smi_bamview *h, uint8_t *out_bgzf, size_t cap, size_t *n_out, uint8_t *out_records, size_t cap_records) {
    if (!h || !n_out || !out_bgzf) {
        set_error("smi_bamview_convert: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed || !h->sized) {
        set_error(h->failed ? "smi_bamview_convert: an earlier call failed" : "smi_bamview_convert: smi_bamview_add_segment comes first");
        return SMI_ERR_STATE;
    }
    size_t bound = 0;
    if (int rc = smi_bgzf_deflate_device(h->ctx, h->d_out, h->n_out, nullptr, 0, &bound)) return rc;
    *n_out = bound;
    if (cap < bound || (out_records && cap_records < h->n_out)) return 1;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    h->ms[SMI_BAMVIEW_MS_GATHER] = h->ms[SMI_BAMVIEW_MS_DEFLATE] = 0.f;
    if (h->n_out) {
        if (int rc = h->ev.begin(s)) return rc;
        hipLaunchKernelGGL(k_view_gather, dim3(view_grid(h->n)), dim3(kViewBlock), 0, s, (const uint8_t *)h->d_bam, (const smi_bam_record *)h->d_recs, (uint32_t)h->n,
                           h->first, (const uint8_t *)h->d_keep, (const uint64_t *)h->d_off, h->d_out);
        SMI_HIP(hipGetLastError());
        if (int rc = h->ev.end(s, &h->ms[SMI_BAMVIEW_MS_GATHER])) return rc;
    }
    if (int rc = h->ev.begin(s)) return rc;
    size_t z = 0;
    if (int rc = smi_bgzf_deflate_device(h->ctx, h->d_out, h->n_out, out_bgzf, cap, &z)) return rc;
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMVIEW_MS_DEFLATE])) return rc;
    if (z < 28) {  // (cannot happen: the deflater closes its stream with the end-of-file block)
        set_error("smi_bamview_convert: the deflater wrote no end-of-file block");
        return SMI_ERR_STATE;
    }
    *n_out = z - 28;  // the caller ends the file
    if (out_records && h->n_out) SMI_HIP(hipMemcpy(out_records, h->d_out, h->n_out, hipMemcpyDeviceToHost));
    if (!h->written) {
        h->counts[SMI_BAMVIEW_RECORDS] += (int64_t)h->n;
        h->counts[SMI_BAMVIEW_KEPT] += (int64_t)h->n_kept;
        h->counts[SMI_BAMVIEW_BYTES] += (int64_t)h->n_bam;
        h->counts[SMI_BAMVIEW_BYTES_KEPT] += (int64_t)h->n_out;
        h->counts[SMI_BAMVIEW_SEGMENTS] += h->n ? 1 : 0;
    }
    h->written = true;
    return SMI_OK;
}

extern "C" int smi_bamview_host_loop(smi_bamview *h, double *seconds, int64_t *mismatches) {
    if (!h || !seconds || !mismatches) {
        set_error("smi_bamview_host_loop: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed || !h->written) {
        set_error(h->failed ? "smi_bamview_host_loop: an earlier call failed" : "smi_bamview_host_loop: smi_bamview_convert comes first");
        return SMI_ERR_STATE;
    }
    *seconds = 0.0;
    *mismatches = 0;
    const size_t n = h->n;
    if (!n) return SMI_OK;
    SMI_HIP(hipSetDevice(h->ctx->device));
    // what the device holds comes to the host (not timed): the bytes, the record index, the keep flags, the offsets and the output
    std::vector<uint8_t> bam(h->n_bam), keep(n), dev(h->n_out);
    std::vector<smi_bam_record> recs(n);
    std::vector<uint64_t> off(n + 1);
    SMI_HIP(hipMemcpy(bam.data(), h->d_bam, h->n_bam, hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(recs.data(), h->d_recs, n * sizeof(smi_bam_record), hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(keep.data(), h->d_keep, n, hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(off.data(), h->d_off, (n + 1) * 8, hipMemcpyDeviceToHost));
    if (h->n_out) SMI_HIP(hipMemcpy(dev.data(), h->d_out, h->n_out, hipMemcpyDeviceToHost));
    Filters f = h->f;
    f.ref_begin = h->ref_begin.data();
    f.ibeg = h->ibeg.data();
    f.iend = h->iend.data();
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> host(h->n_out), mine(n);
    std::vector<uint64_t> at(n + 1);
    uint64_t to = 0;
    for (size_t i = 0; i < n; i++) {
        const smi_bam_record &r = recs[i];
        unsigned long long sum = 0;
        if (f.has_regions) {
            const uint8_t *c = bam.data() + (r.cigar_off - h->first);
            for (uint32_t k = 0; k < r.n_cigar; k++) {
                uint32_t w;
                std::memcpy(&w, c + 4ull * k, 4);
                if (on_reference(w)) sum += w >> 4;
            }
        }
        mine[i] = r.ref_id < h->n_ref && view_keep(f, r.flag, r.mapq, r.ref_id, r.pos, r.n_cigar, sum);
        at[i] = to;
        if (mine[i] && to + r.rec_len <= host.size()) std::memcpy(host.data() + to, bam.data() + (r.rec_off - h->first), r.rec_len);
        if (mine[i]) to += r.rec_len;
    }
    at[n] = to;
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    int64_t bad = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t len = at[i + 1] - at[i];
        if (mine[i] != keep[i] || off[i + 1] - off[i] != len || off[i] != at[i] || at[i] + len > host.size() || off[i] + len > dev.size() ||
            std::memcmp(dev.data() + off[i], host.data() + at[i], len))
            bad++;
    }
    *mismatches = bad;
    return SMI_OK;
}
