// smi_bamsort.hip -- `BamSort`: the coordinate sort of a BAM, in the place of `samtools sort`.  The order is this build's own canonical
// definition (tests/sortmodel.py restates it): reference rank (a negative ref_id ranks behind the header's
// references), pos + 1 as an unsigned number, the reverse-strand bit; records with equal keys keep their input order.
//
// The caller hands in the inflated stream in segments with their record index (smi_bamsort_add_segment).  The record bytes of every
// segment stay resident in one device arena; per segment
//   K-SORT-KEY     one lane per record: the 64-bit key, the record's 64-bit arena offset and its 32-bit length; a ref_id outside the
//                  header stops the run (atomicMin of the record number)
// at smi_bamsort_finish: one stable hipcub radix sort of key -> record ordinal over the key's significant bits, K-SORT-PERM (the lengths
// in sorted order), a hipcub exclusive scan (the 64-bit output offset of every rank) and K-SORT-WINDOWS (the borders of the output windows,
// found on the device: the offsets never leave it); and per window (smi_bamsort_window)
//   K-SORT-GATHER  kSortLanes lanes per record copy it from the arena to the window buffer: the destination in aligned 16-byte stores,
//                  the source through unaligned 16-byte loads, head and tail one byte per lane
// and the library's BGZF deflater (smi_bgzf_deflate_device) on the window buffer.
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "smi_device.h"
#include "smi_handle.h"
#include "smi_internal.h"

namespace smi {
namespace {

constexpr int kSortBlock = 256;
constexpr int kSortLanes = 16;  // lanes per record of K-SORT-GATHER (why 16)
constexpr int kSortRecs = kSortBlock / kSortLanes;
constexpr unsigned long long kNoRecord = ~0ull;
// device bytes per record beside the arena: key 8, arena offset 8, length 4 for the whole run; at finish the sorted keys 8, the
// ordinals in and out 4 + 4, the output offsets 8 and the sort's own storage (about 4)
constexpr uint64_t kPerRecord = SMI_BAMSORT_PER_RECORD;

__global__ __launch_bounds__(kSortBlock) void k_sort_key(const smi_bam_record *__restrict__ recs, uint32_t n, int32_t n_ref, uint64_t first, uint64_t arena_at,
                                                         unsigned long long *__restrict__ key, uint64_t *__restrict__ off, uint32_t *__restrict__ len,
                                                         unsigned long long *__restrict__ stop) {
    const uint32_t i = blockIdx.x * kSortBlock + threadIdx.x;
    if (i >= n) return;
    const smi_bam_record *r = recs + i;
    const int32_t ref = r->ref_id;
    if (ref >= n_ref) atomicMin(stop, (unsigned long long)i);
    const unsigned long long rank = ref < 0 || ref >= n_ref ? (uint32_t)n_ref : (uint32_t)ref;
    key[i] = rank << 33 | (unsigned long long)((uint32_t)r->pos + 1u) << 1 | ((r->flag >> 4) & 1u);
    off[i] = arena_at + (r->rec_off - first);
    len[i] = r->rec_len;
}

__global__ __launch_bounds__(kSortBlock) void k_sort_iota(uint32_t *__restrict__ ord, uint32_t n) {
    const uint32_t i = blockIdx.x * kSortBlock + threadIdx.x;
    if (i < n) ord[i] = i;
}

// the lengths in sorted order, as the 64-bit numbers the scan sums in place; entry n takes the total
__global__ __launch_bounds__(kSortBlock) void k_sort_perm(const uint32_t *__restrict__ ord, const uint32_t *__restrict__ len, uint32_t n, uint64_t *__restrict__ ooff) {
    const uint32_t r = blockIdx.x * kSortBlock + threadIdx.x;
    if (r < n) ooff[r] = len[ord[r]];
    else if (r == n) ooff[r] = 0;
}

// K-SORT-WINDOWS: one lane walks the windows; window k holds the ranks [rank[k], rank[k + 1]): as many whole records as window_bytes
// hold, at least one.  A window and the record behind it exceed window_bytes, so there are at most 2 * total / window_bytes + 1 windows.
__global__ void k_sort_windows(const uint64_t *__restrict__ ooff, uint32_t n, uint64_t window_bytes, uint32_t cap, uint32_t *__restrict__ rank,
                               uint64_t *__restrict__ byte, uint32_t *__restrict__ n_windows) {
    uint32_t b = 0, k = 0;
    while (b < n && k < cap) {
        const uint64_t lim = ooff[b] + window_bytes;
        uint32_t lo = b + 1, hi = n;  // the largest e in [b + 1, n] with ooff[e] <= lim, or b + 1
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (ooff[mid] <= lim) lo = mid;
            else hi = mid - 1;
        }
        rank[k] = b;
        byte[k] = ooff[b];
        k++;
        b = lo;
    }
    rank[k] = n;
    byte[k] = ooff[n];
    *n_windows = b < n ? 0xffffffffu : k;  // (cannot happen: cap holds the bound above)
}

template <int W>
struct Word;
template <>
struct Word<16> {
    using type = uint4;
};
template <>
struct Word<4> {
    using type = uint32_t;
};

// K-SORT-GATHER: the records of the ranks [r0, r0 + n) from the arena to dst, which begins at output offset `base` and is aligned to 256
// bytes.  kSortLanes lanes share a record: the bytes in front of the first W-aligned destination address and those behind the last one go
// one byte per lane (fewer than W <= kSortLanes of either), the body in W-byte words: a store aligned to W, a load of any alignment.
// Every load and store lies inside the record.
template <int W>
__global__ __launch_bounds__(kSortBlock) void k_sort_gather(const uint8_t *__restrict__ arena, const uint64_t *__restrict__ off, const uint32_t *__restrict__ len,
                                                            const uint32_t *__restrict__ ord, const uint64_t *__restrict__ ooff, uint32_t r0, uint32_t n, uint64_t base,
                                                            uint8_t *__restrict__ dst) {
    using T = typename Word<W>::type;
    static_assert(W <= kSortLanes, "head and tail go one byte per lane");
    const uint32_t g = blockIdx.x * kSortRecs + threadIdx.x / kSortLanes, sub = threadIdx.x % kSortLanes;
    if (g >= n) return;
    const uint32_t i = ord[r0 + g];
    const uint8_t *__restrict__ s = arena + off[i];
    const uint32_t L = len[i];
    const uint64_t d0 = ooff[r0 + g] - base;
    uint8_t *__restrict__ d = dst + d0;
    const uint32_t want = (uint32_t)(-(int64_t)d0) & (W - 1), head = want < L ? want : L;
    const uint32_t words = (L - head) / W, tail = (L - head) % W, tail_at = head + words * W;
    if (sub < head) d[sub] = s[sub];
    for (uint32_t w = sub; w < words; w += kSortLanes) {
        T v;
        __builtin_memcpy(&v, s + head + (size_t)w * W, W);
        *reinterpret_cast<T *>(__builtin_assume_aligned(d + head + (size_t)w * W, W)) = v;
    }
    if (sub < tail) d[tail_at + sub] = s[tail_at + sub];
}

template <class T>
int sort_grow(T **p, size_t &cap, size_t want) {
    if (want <= cap && *p) return SMI_OK;
    const size_t n = std::max<size_t>(want + want / 4, 1024);
    if (*p) SMI_HIP(hipFree(*p));
    *p = nullptr;
    cap = 0;
    SMI_HIP(hipMalloc((void **)p, n * sizeof(T)));
    cap = n;
    return SMI_OK;
}

// a device array of at least `want` elements (at most `limit` are asked for when that holds them) whose first `used` elements are kept
template <class T>
int sort_grow_keep(T **p, size_t &cap, size_t used, size_t want, size_t limit, hipStream_t s) {
    if (want <= cap && *p) return SMI_OK;
    size_t n = std::max<size_t>(std::max(want, 2 * cap), 1024);
    if (limit >= want) n = std::min(n, std::max<size_t>(limit, 1024));
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

inline unsigned sort_grid(size_t n, unsigned per = kSortBlock) { return (unsigned)std::max<size_t>(1, (n + per - 1) / per); }

inline uint64_t host_key(const uint8_t *rec, int32_t n_ref) {
    int32_t ref, pos;
    uint16_t flag;
    std::memcpy(&ref, rec + 4, 4);
    std::memcpy(&pos, rec + 8, 4);
    std::memcpy(&flag, rec + 18, 2);
    const uint64_t rank = ref < 0 || ref >= n_ref ? (uint32_t)n_ref : (uint32_t)ref;
    return rank << 33 | (uint64_t)((uint32_t)pos + 1u) << 1 | ((flag >> 4) & 1u);
}

}  // namespace
}  // namespace smi

using namespace smi;

struct smi_bamsort {
    smi_ctx *ctx = nullptr;
    int32_t n_ref = 0;
    uint64_t resident_bytes = 0, window_bytes = 0;
    int store_bytes = 16;  // SMI_BAMSORT_STORE_BYTES=4: the gather in 4-byte words (measurement; the same bytes)
    // resident: the arena and the per-record arrays
    uint8_t *d_arena = nullptr;
    size_t arena_cap = 0, arena_used = 0;
    unsigned long long *d_key = nullptr;
    uint64_t *d_off = nullptr;
    uint32_t *d_len = nullptr;
    size_t key_cap = 0, off_cap = 0, len_cap = 0;
    uint64_t n_records = 0;
    // one segment (grow-only)
    smi_bam_record *d_recs = nullptr;
    size_t recs_cap = 0;
    unsigned long long *d_stop = nullptr;
    // after finish
    uint32_t *d_ord = nullptr;   // the record ordinal of every rank
    uint64_t *d_ooff = nullptr;  // [n + 1] the output offset of every rank, and the total
    uint8_t *d_win = nullptr;
    size_t win_cap = 0;
    std::vector<uint32_t> win_rank;  // [n_windows + 1]
    std::vector<uint64_t> win_byte;
    Events ev;
    int64_t counts[SMI_BAMSORT_N_COUNT] = {};
    float ms[SMI_BAMSORT_N_STAGE] = {};
    std::string error_read;
    int64_t error_record = -1;
    bool failed = false, finished = false;
};

namespace {

void sort_release(smi_bamsort *h) {
    void *bufs[] = {h->d_arena, h->d_key, h->d_off, h->d_len, h->d_recs, h->d_stop, h->d_ord, h->d_ooff, h->d_win};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    delete h;
}

int sort_too_large(smi_bamsort *h) {
    h->failed = true;
    set_error("BamSort: the BAM inflates to more than " + std::to_string(h->resident_bytes) +
              " bytes; this build sorts a BAM that is resident in device memory");
    return SMI_ERR_INVALID;
}

int sort_gather(smi_bamsort *h, size_t k) {
    const uint32_t r0 = h->win_rank[k], n = h->win_rank[k + 1] - r0;
    hipStream_t s = h->ctx->stream;
    if (h->store_bytes == 4)
        hipLaunchKernelGGL(k_sort_gather<4>, dim3(sort_grid(n, kSortRecs)), dim3(kSortBlock), 0, s, (const uint8_t *)h->d_arena, (const uint64_t *)h->d_off,
                           (const uint32_t *)h->d_len, (const uint32_t *)h->d_ord, (const uint64_t *)h->d_ooff, r0, n, h->win_byte[k], h->d_win);
    else
        hipLaunchKernelGGL(k_sort_gather<16>, dim3(sort_grid(n, kSortRecs)), dim3(kSortBlock), 0, s, (const uint8_t *)h->d_arena, (const uint64_t *)h->d_off,
                           (const uint32_t *)h->d_len, (const uint32_t *)h->d_ord, (const uint64_t *)h->d_ooff, r0, n, h->win_byte[k], h->d_win);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

}  // namespace

extern "C" int smi_bamsort_create(smi_ctx *ctx, int32_t n_ref, uint64_t resident_bytes, uint64_t window_bytes, smi_bamsort **out) {
    if (!ctx || !out || n_ref < 0 || !window_bytes) {
        set_error("smi_bamsort_create: bad argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    SMI_HIP(hipSetDevice(ctx->device));
    if (!resident_bytes) {  // two fifths of what is free: the arena grows by a copy, so old and new stand side by side for a moment
        size_t free_b = 0, total_b = 0;
        SMI_HIP(hipMemGetInfo(&free_b, &total_b));
        resident_bytes = (uint64_t)free_b / 5 * 2;
    }
    smi_bamsort *h = new smi_bamsort();
    h->ctx = ctx;
    h->n_ref = n_ref;
    h->resident_bytes = resident_bytes;
    h->window_bytes = window_bytes;
    if (const char *e = std::getenv("SMI_BAMSORT_STORE_BYTES"))
        if (std::atoi(e) == 4) h->store_bytes = 4;
    hipError_t e = hipMalloc((void **)&h->d_stop, sizeof(unsigned long long));
    if (e != hipSuccess) {
        sort_release(h);
        return hip_fail(e, "smi_bamsort_create");
    }
    *out = h;
    return SMI_OK;
}

extern "C" int smi_bamsort_free(smi_bamsort *h) {
    if (h) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        sort_release(h);
    }
    return SMI_OK;
}

extern "C" int smi_bamsort_counts(const smi_bamsort *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_bamsort_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof h->counts);
    return SMI_OK;
}

extern "C" int smi_bamsort_stage_ms(const smi_bamsort *h, float *ms) {
    if (!h || !ms) {
        set_error("smi_bamsort_stage_ms: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(ms, h->ms, sizeof h->ms);
    return SMI_OK;
}

extern "C" int smi_bamsort_error_read(const smi_bamsort *h, char *name, size_t cap, int64_t *record) {
    if (!h || !record || (cap && !name)) {
        set_error("smi_bamsort_error_read: null argument");
        return SMI_ERR_INVALID;
    }
    return handle::error_read(h->error_read, h->error_record, name, cap, record);
}

extern "C" int smi_bamsort_add_segment(smi_bamsort *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n) {
    if (!h || n < 0 || (n && (!bam || !recs))) {
        set_error("smi_bamsort_add_segment: bad argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed || h->finished) {
        set_error(h->failed ? "smi_bamsort_add_segment: an earlier call failed" : "smi_bamsort_add_segment: the sort is finished");
        return SMI_ERR_STATE;
    }
    if (!n) return SMI_OK;
    const size_t N = (size_t)n;
    // every record inside the buffer, the records one behind the other: the arena takes bam[first .. last) and the gather reads nothing else
    for (int32_t i = 0; i < n; i++) {
        const smi_bam_record &r = recs[i];
        if (r.rec_len < 36 || r.rec_off + r.rec_len > n_bam || r.name_off < r.rec_off || r.name_off + r.l_read_name > r.rec_off + r.rec_len ||
            (i && r.rec_off < recs[i - 1].rec_off + recs[i - 1].rec_len)) {
            set_error("smi_bamsort_add_segment: record index entry " + std::to_string(i) + " points outside the BAM buffer");
            return SMI_ERR_INVALID;
        }
    }
    if (h->n_records + N > (uint64_t)INT32_MAX) {  // hipcub counts in int
        h->failed = true;
        set_error("BamSort: more than 2^31 - 1 records");
        return SMI_ERR_INVALID;
    }
    const uint64_t first = recs[0].rec_off, last = recs[n - 1].rec_off + recs[n - 1].rec_len;
    const size_t bytes = (size_t)(last - first), total = (size_t)h->n_records + N;
    if (h->arena_used + bytes + kPerRecord * total > h->resident_bytes) return sort_too_large(h);
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    std::memset(h->ms, 0, sizeof h->ms);
    const size_t arena_limit = (size_t)(h->resident_bytes - kPerRecord * total);
    if (int rc = sort_grow_keep(&h->d_arena, h->arena_cap, h->arena_used, h->arena_used + bytes, arena_limit, s)) return rc;
    if (int rc = sort_grow_keep(&h->d_key, h->key_cap, (size_t)h->n_records, total, 0, s)) return rc;
    if (int rc = sort_grow_keep(&h->d_off, h->off_cap, (size_t)h->n_records, total, 0, s)) return rc;
    if (int rc = sort_grow_keep(&h->d_len, h->len_cap, (size_t)h->n_records, total, 0, s)) return rc;
    if (int rc = sort_grow(&h->d_recs, h->recs_cap, N)) return rc;
    h->failed = true;  // until the segment is through
    SMI_HIP(hipMemcpyAsync(h->d_arena + h->arena_used, bam + first, bytes, hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemcpyAsync(h->d_recs, recs, N * sizeof(smi_bam_record), hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemsetAsync(h->d_stop, 0xff, sizeof(unsigned long long), s));
    if (int rc = h->ev.begin(s)) return rc;
    hipLaunchKernelGGL(k_sort_key, dim3(sort_grid(N)), dim3(kSortBlock), 0, s, (const smi_bam_record *)h->d_recs, (uint32_t)n, h->n_ref, first, (uint64_t)h->arena_used,
                       h->d_key + h->n_records, h->d_off + h->n_records, h->d_len + h->n_records, h->d_stop);
    SMI_HIP(hipGetLastError());
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMSORT_MS_KEY])) return rc;
    unsigned long long stop = kNoRecord;
    SMI_HIP(hipMemcpyAsync(&stop, h->d_stop, sizeof stop, hipMemcpyDeviceToHost, s));
    SMI_HIP(hipStreamSynchronize(s));
    if (stop != kNoRecord) {
        const smi_bam_record &r = recs[stop];
        h->error_read.assign((const char *)bam + r.name_off, r.l_read_name ? r.l_read_name - 1u : 0u);
        h->error_record = (int64_t)h->n_records + (int64_t)stop;
        set_error("read " + h->error_read + " (record " + std::to_string(h->error_record) + "): its ref_id is not one of the header's references");
        return 2;
    }
    h->arena_used += bytes;
    h->n_records = total;
    h->counts[SMI_BAMSORT_RECORDS] = (int64_t)total;
    h->counts[SMI_BAMSORT_SEGMENTS]++;
    h->counts[SMI_BAMSORT_ARENA_BYTES] = (int64_t)h->arena_used;
    h->counts[SMI_BAMSORT_ARENA_HELD] = (int64_t)h->arena_cap;
    h->failed = false;
    return SMI_OK;
}

namespace {

int sort_finish(smi_bamsort *h) {
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    const size_t n = (size_t)h->n_records;
    std::memset(h->ms, 0, sizeof h->ms);
    h->win_rank.assign(1, 0);
    h->win_byte.assign(1, 0);
    if (!n) return SMI_OK;
    // at most 2 * total / window_bytes + 1 windows (K-SORT-WINDOWS), and no more than records
    const size_t cap_w = (size_t)std::min<uint64_t>(n, 2 * (uint64_t)h->arena_used / h->window_bytes + 2);
    DevBuf<unsigned long long> skey("BamSort");
    DevBuf<uint32_t> iota("BamSort"), wrank("BamSort"), nwin("BamSort");
    DevBuf<uint64_t> wbyte("BamSort");
    Scratch cub("BamSort");
    if (int rc = skey.alloc(n)) return rc;
    if (int rc = iota.alloc(n)) return rc;
    if (int rc = wrank.alloc(cap_w + 1)) return rc;
    if (int rc = wbyte.alloc(cap_w + 1)) return rc;
    if (int rc = nwin.alloc(1)) return rc;
    SMI_HIP(hipMalloc((void **)&h->d_ord, n * sizeof(uint32_t)));
    SMI_HIP(hipMalloc((void **)&h->d_ooff, (n + 1) * sizeof(uint64_t)));
    int ref_bits = 1;  // the ranks 0 .. n_ref
    while (ref_bits < 31 && (1ll << ref_bits) <= h->n_ref) ref_bits++;
    const auto sort = [&](void *p, size_t &t) { return hipcub::DeviceRadixSort::SortPairs(p, t, h->d_key, skey.p, iota.p, h->d_ord, (int)n, 0, 33 + ref_bits, s); };
    const auto offsets = [&](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, h->d_ooff, h->d_ooff, (int)(n + 1), s); };
    if (int rc = reserve(cub, sort, offsets)) return rc;
    if (int rc = h->ev.begin(s)) return rc;
    hipLaunchKernelGGL(k_sort_iota, dim3(sort_grid(n)), dim3(kSortBlock), 0, s, iota.p, (uint32_t)n);
    SMI_HIP(hipGetLastError());
    if (int rc = run_reserved(cub, sort)) return rc;
    hipLaunchKernelGGL(k_sort_perm, dim3(sort_grid(n + 1)), dim3(kSortBlock), 0, s, (const uint32_t *)h->d_ord, (const uint32_t *)h->d_len, (uint32_t)n, h->d_ooff);
    SMI_HIP(hipGetLastError());
    if (int rc = run_reserved(cub, offsets)) return rc;
    hipLaunchKernelGGL(k_sort_windows, dim3(1), dim3(1), 0, s, (const uint64_t *)h->d_ooff, (uint32_t)n, h->window_bytes, (uint32_t)cap_w, wrank.p, wbyte.p, nwin.p);
    SMI_HIP(hipGetLastError());
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMSORT_MS_SORT])) return rc;
    uint32_t nw = 0;
    SMI_HIP(hipMemcpy(&nw, nwin.p, sizeof nw, hipMemcpyDeviceToHost));
    if (nw == 0xffffffffu || nw > cap_w) {  // (cannot happen)
        set_error("BamSort: more windows than their bound");
        return SMI_ERR_STATE;
    }
    h->win_rank.resize((size_t)nw + 1);
    h->win_byte.resize((size_t)nw + 1);
    SMI_HIP(hipMemcpy(h->win_rank.data(), wrank.p, ((size_t)nw + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(h->win_byte.data(), wbyte.p, ((size_t)nw + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (h->win_rank[nw] != n || h->win_byte[nw] != h->arena_used) {  // (cannot happen: the lengths sum to the arena's bytes)
        set_error("BamSort: the windows do not add up to the records taken");
        return SMI_ERR_STATE;
    }
    // the keys have done their work
    SMI_HIP(hipFree(h->d_key));
    h->d_key = nullptr;
    h->key_cap = 0;
    uint64_t largest = 0;
    for (size_t k = 0; k < nw; k++) largest = std::max(largest, h->win_byte[k + 1] - h->win_byte[k]);
    SMI_HIP(hipMalloc((void **)&h->d_win, (size_t)largest + 256));
    h->win_cap = (size_t)largest;
    h->counts[SMI_BAMSORT_WINDOWS] = nw;
    h->counts[SMI_BAMSORT_LARGEST_WINDOW] = (int64_t)largest;
    return SMI_OK;
}

}  // namespace

extern "C" int smi_bamsort_finish(smi_bamsort *h, int64_t *n_windows, int64_t *n_records) {
    if (!h || !n_windows || !n_records) {
        set_error("smi_bamsort_finish: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed) {
        set_error("smi_bamsort_finish: an earlier call failed");
        return SMI_ERR_STATE;
    }
    if (!h->finished) {
        if (int rc = sort_finish(h)) {
            h->failed = true;
            return rc;
        }
        h->finished = true;
    }
    *n_windows = (int64_t)h->win_rank.size() - 1;
    *n_records = (int64_t)h->n_records;
    return SMI_OK;
}

extern "C" int smi_bamsort_window(smi_bamsort *h, int64_t k, uint8_t *out_bgzf, size_t cap, size_t *n_out, uint8_t *out_inflated, size_t cap_inflated,
                                  size_t *n_inflated) {
    if (!h || !n_out || !n_inflated) {
        set_error("smi_bamsort_window: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed || !h->finished) {
        set_error(h->failed ? "smi_bamsort_window: an earlier call failed" : "smi_bamsort_window: smi_bamsort_finish comes first");
        return SMI_ERR_STATE;
    }
    if (k < 0 || (size_t)k + 1 >= h->win_rank.size()) {
        set_error("smi_bamsort_window: no window " + std::to_string(k));
        return SMI_ERR_INVALID;
    }
    const size_t bytes = (size_t)(h->win_byte[k + 1] - h->win_byte[k]);
    size_t bound = 0;
    if (int rc = smi_bgzf_deflate_device(h->ctx, h->d_win, bytes, nullptr, 0, &bound)) return rc;
    *n_out = bound;
    *n_inflated = bytes;
    if (!out_bgzf) return SMI_OK;
    if (cap < bound || (out_inflated && cap_inflated < bytes)) return 1;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    std::memset(h->ms, 0, sizeof h->ms);
    if (int rc = h->ev.begin(s)) return rc;
    if (int rc = sort_gather(h, (size_t)k)) return rc;
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMSORT_MS_GATHER])) return rc;
    if (int rc = h->ev.begin(s)) return rc;
    size_t z = 0;
    if (int rc = smi_bgzf_deflate_device(h->ctx, h->d_win, bytes, out_bgzf, cap, &z)) return rc;
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMSORT_MS_DEFLATE])) return rc;
    if (z < 28) {  // (cannot happen: the deflater closes its stream with the end-of-file block)
        set_error("smi_bamsort_window: the deflater wrote no end-of-file block");
        return SMI_ERR_STATE;
    }
    *n_out = z - 28;  // the caller ends the file
    if (out_inflated) SMI_HIP(hipMemcpy(out_inflated, h->d_win, bytes, hipMemcpyDeviceToHost));
    h->counts[SMI_BAMSORT_BYTES_OUT] += (int64_t)bytes;
    return SMI_OK;
}

extern "C" int smi_bamsort_host_loop(smi_bamsort *h, double *seconds, int64_t *mismatches) {
    if (!h || !seconds || !mismatches) {
        set_error("smi_bamsort_host_loop: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed || !h->finished) {
        set_error(h->failed ? "smi_bamsort_host_loop: an earlier call failed" : "smi_bamsort_host_loop: smi_bamsort_finish comes first");
        return SMI_ERR_STATE;
    }
    SMI_HIP(hipSetDevice(h->ctx->device));
    const size_t n = (size_t)h->n_records;
    *seconds = 0.0;
    *mismatches = 0;
    if (!n) return SMI_OK;
    // what the device holds comes to the host (not timed): the arena, and where every record lies in it
    std::vector<uint8_t> arena(h->arena_used), sorted(h->arena_used), win(h->win_cap);
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> len(n);
    SMI_HIP(hipMemcpy(arena.data(), h->d_arena, h->arena_used, hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(off.data(), h->d_off, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(len.data(), h->d_len, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> key(n), at(n);
    std::vector<uint32_t> ord(n);
    for (size_t i = 0; i < n; i++) key[i] = host_key(arena.data() + off[i], h->n_ref);
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    uint64_t o = 0;
    for (size_t r = 0; r < n; r++) {
        at[r] = o;
        std::memcpy(sorted.data() + o, arena.data() + off[ord[r]], len[ord[r]]);
        o += len[ord[r]];
    }
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // the device's output, window by window, against it
    hipStream_t s = h->ctx->stream;
    int64_t bad = 0;
    for (size_t k = 0; k + 1 < h->win_rank.size(); k++) {
        const size_t bytes = (size_t)(h->win_byte[k + 1] - h->win_byte[k]);
        if (int rc = sort_gather(h, k)) return rc;
        SMI_HIP(hipMemcpyAsync(win.data(), h->d_win, bytes, hipMemcpyDeviceToHost, s));
        SMI_HIP(hipStreamSynchronize(s));
        for (uint32_t r = h->win_rank[k]; r < h->win_rank[k + 1]; r++) {
            const uint64_t w = at[r] - h->win_byte[k];
            if (at[r] < h->win_byte[k] || w + len[ord[r]] > bytes || std::memcmp(win.data() + w, sorted.data() + at[r], len[ord[r]])) bad++;
        }
    }
    *mismatches = bad;
    return SMI_OK;
}
