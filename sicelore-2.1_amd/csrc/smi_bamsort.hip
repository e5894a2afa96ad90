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
//
// Run mode (smi_bamsort_run_mode) sorts a file beyond resident_bytes.  A segment that does not fit makes add_segment answer 3; the caller
// then spills: smi_bamsort_spill_begin sorts what the arena holds with the machinery above, smi_bamsort_spill_window hands out the run's
// windows as raw bytes for the caller's run file, smi_bamsort_spill_end empties the arena.  Of every spilled record the device keeps, in
// its run's sorted order, the key, the length and the byte offset in the run file.  smi_bamsort_finish then sorts the keys of all runs
// once more (stable, so ties stand in run order and inside a run in input order: the input's order), and
//   K-MERGE-RANK    rank_of[ord[r]] = r, monotone inside a run
//   K-MERGE-SLICES  one lane per (window border, run): the first ordinal of the run at or behind the border, by binary search in rank_of,
//                   and its byte offset in the run file: every window draws one contiguous slice from each run
// and per window (smi_bamsort_merge_window) the caller's concatenated slices are uploaded to a staging buffer and
//   K-MERGE-GATHER  K-SORT-GATHER's copy with the source in the staging buffer: the record's run by a search in the table of first
//                   ordinals, its address the run-file offset moved by the run's slice
// fills the window buffer for the deflater.
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
// ordinals in and out 4 + 4, the output offsets 8 and the sort's own storage (about 4).  Run mode stays inside it: a spilled record keeps
// 20 (key, length, run-file offset); a spill writes those 20 where they stay, beside the arena's 20, the ordinals 4 and the sort's storage
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

static_assert(kSortLanes == kCopyLanes, "copy_record (smi_device.h) shares a record among kCopyLanes lanes");

// K-SORT-GATHER: the records of the ranks [r0, r0 + n) from the arena to dst, which begins at output offset `base` and is aligned to 256
// bytes.  kSortLanes lanes share a record (copy_record).
template <int W>
__global__ __launch_bounds__(kSortBlock) void k_sort_gather(const uint8_t *__restrict__ arena, const uint64_t *__restrict__ off, const uint32_t *__restrict__ len,
                                                            const uint32_t *__restrict__ ord, const uint64_t *__restrict__ ooff, uint32_t r0, uint32_t n, uint64_t base,
                                                            uint8_t *__restrict__ dst) {
    const uint32_t g = blockIdx.x * kSortRecs + threadIdx.x / kSortLanes, sub = threadIdx.x % kSortLanes;
    if (g >= n) return;
    const uint32_t i = ord[r0 + g];
    copy_record<W>(arena + off[i], len[i], ooff[r0 + g] - base, dst, sub);
}

// the lengths of a run in its sorted order, kept for the merge (they take the place of the sort's iota, which has done its work)
__global__ __launch_bounds__(kSortBlock) void k_run_len(const uint32_t *__restrict__ ord, const uint32_t *__restrict__ len, uint32_t n, uint32_t *__restrict__ slen) {
    const uint32_t r = blockIdx.x * kSortBlock + threadIdx.x;
    if (r < n) slen[r] = len[ord[r]];
}

// K-MERGE-RANK: the inverse of the global order.  The ordinals of a run stand in its sorted order, so rank_of rises inside a run.
__global__ __launch_bounds__(kSortBlock) void k_merge_rank(const uint32_t *__restrict__ ord, uint32_t n, uint32_t *__restrict__ rank_of) {
    const uint32_t r = blockIdx.x * kSortBlock + threadIdx.x;
    if (r < n) rank_of[ord[r]] = r;
}

// K-MERGE-SLICES: one lane per (window border b, run j): the first ordinal of run j whose rank is not in front of the border, and that
// record's byte offset in the run file (the run's size where there is none).  Window k draws the bytes between its two borders from run j.
__global__ __launch_bounds__(kSortBlock) void k_merge_slices(const uint32_t *__restrict__ rank_of, const uint64_t *__restrict__ roff,
                                                             const uint32_t *__restrict__ run_first, const uint64_t *__restrict__ run_bytes,
                                                             const uint32_t *__restrict__ win_rank, uint64_t n_entries, uint32_t n_runs,
                                                             uint32_t *__restrict__ slice_ord, uint64_t *__restrict__ slice_byte) {
    const uint64_t t = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x;
    if (t >= n_entries) return;
    const uint32_t j = (uint32_t)(t % n_runs), border = win_rank[t / n_runs], end = run_first[j + 1];
    uint32_t lo = run_first[j], hi = end;  // the first i in [lo, hi) with rank_of[i] >= border, or hi
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rank_of[mid] < border) lo = mid + 1;
        else hi = mid;
    }
    slice_ord[t] = lo;
    slice_byte[t] = lo < end ? roff[lo] : run_bytes[j];
}

// K-MERGE-GATHER: the records of the ranks [r0, r0 + n) from the staging buffer, which holds the window's slice of every run one behind
// the other, to dst.  A record's run is the last one whose first ordinal is not behind the record's (a search of the group in run_first:
// n_runs + 1 entries, read by every group, so they stay in the caches), and its source is its run-file offset moved by delta[run] = where
// the run's slice begins in the staging buffer minus where it begins in the run file.  A source outside the staging buffer (cannot
// happen: the slices are the windows' own) is not read; the rank is reported in *bad.
template <int W>
__global__ __launch_bounds__(kSortBlock) void k_merge_gather(const uint8_t *__restrict__ stage, uint64_t stage_bytes, const uint64_t *__restrict__ roff,
                                                             const uint32_t *__restrict__ ord, const uint64_t *__restrict__ ooff,
                                                             const uint32_t *__restrict__ run_first, uint32_t n_runs, const int64_t *__restrict__ delta, uint32_t r0,
                                                             uint32_t n, uint64_t base, uint8_t *__restrict__ dst, unsigned long long *__restrict__ bad) {
    const uint32_t g = blockIdx.x * kSortRecs + threadIdx.x / kSortLanes, sub = threadIdx.x % kSortLanes;
    if (g >= n) return;
    const uint32_t i = ord[r0 + g];
    const uint64_t o = ooff[r0 + g];
    const uint32_t L = (uint32_t)(ooff[r0 + g + 1] - o);
    uint32_t lo = 0, hi = n_runs - 1;  // the largest j with run_first[j] <= i
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (run_first[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const uint64_t at = roff[i] + (uint64_t)delta[lo];
    if (at > stage_bytes || L > stage_bytes - at) {
        if (!sub) atomicMin(bad, (unsigned long long)(r0 + g));
        return;
    }
    copy_record<W>(stage + at, L, o - base, dst, sub);
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
    // run mode: of every spilled record, in its run's sorted order, the key, the length and the byte offset in the run file
    bool run_mode = false, spilling = false;
    unsigned long long *d_rkey = nullptr;
    uint32_t *d_rlen = nullptr;
    uint64_t *d_roff = nullptr;  // one entry more than records: a spill's scan leaves its total there
    size_t rkey_cap = 0, rlen_cap = 0, roff_cap = 0;
    uint64_t n_spilled = 0;            // records in runs; the arena holds the ordinals n_spilled .. n_records
    std::vector<uint32_t> run_first;   // [runs + 1] the first ordinal of every run
    std::vector<uint64_t> run_bytes;   // [runs] the size of every run file
    uint64_t spilled_bytes = 0;
    // run mode after finish
    uint32_t *d_run_first = nullptr;
    int64_t *d_delta = nullptr;
    uint8_t *d_stage = nullptr;
    std::vector<uint32_t> slice_ord;   // [(n_windows + 1) * runs] K-MERGE-SLICES' table, border-major
    std::vector<uint64_t> slice_byte;
    std::vector<int64_t> delta;
    Events ev;
    int64_t counts[SMI_BAMSORT_N_COUNT] = {};
    float ms[SMI_BAMSORT_N_STAGE] = {};
    std::string error_read;
    int64_t error_record = -1;
    bool failed = false, finished = false;
};

namespace {

void sort_release(smi_bamsort *h) {
    void *bufs[] = {h->d_arena, h->d_key, h->d_off, h->d_len, h->d_recs, h->d_stop, h->d_ord, h->d_ooff, h->d_win, h->d_rkey, h->d_rlen, h->d_roff,
                    h->d_run_first, h->d_delta, h->d_stage};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    delete h;
}

template <class T>
int sort_drop(T **p, size_t *cap = nullptr) {
    if (*p) SMI_HIP(hipFree(*p));
    *p = nullptr;
    if (cap) *cap = 0;
    return SMI_OK;
}

int sort_segment_too_large(smi_bamsort *h, size_t bytes, size_t total) {
    h->failed = true;
    set_error("BamSort: a segment of " + std::to_string(bytes) + " record bytes and the per-record arrays of the " + std::to_string(total) +
              " records taken so far exceed resident_bytes = " + std::to_string(h->resident_bytes) +
              ", so it cannot become a run: lower segment_bytes or raise resident_bytes");
    return SMI_ERR_INVALID;
}

int sort_too_large(smi_bamsort *h) {
    h->failed = true;
    set_error("BamSort: the BAM inflates to more than " + std::to_string(h->resident_bytes) +
              " bytes; this build sorts a BAM that is resident in device memory");
    return SMI_ERR_INVALID;
}

// window k of the arena's records; ooff: the output offsets its borders were found in (h->d_ooff, or a run's own while it is spilled)
int sort_gather(smi_bamsort *h, size_t k, const uint64_t *ooff) {
    const uint32_t r0 = h->win_rank[k], n = h->win_rank[k + 1] - r0;
    hipStream_t s = h->ctx->stream;
    if (h->store_bytes == 4)
        hipLaunchKernelGGL(k_sort_gather<4>, dim3(sort_grid(n, kSortRecs)), dim3(kSortBlock), 0, s, (const uint8_t *)h->d_arena, (const uint64_t *)h->d_off,
                           (const uint32_t *)h->d_len, (const uint32_t *)h->d_ord, ooff, r0, n, h->win_byte[k], h->d_win);
    else
        hipLaunchKernelGGL(k_sort_gather<16>, dim3(sort_grid(n, kSortRecs)), dim3(kSortBlock), 0, s, (const uint8_t *)h->d_arena, (const uint64_t *)h->d_off,
                           (const uint32_t *)h->d_len, (const uint32_t *)h->d_ord, ooff, r0, n, h->win_byte[k], h->d_win);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

bool sort_merging(const smi_bamsort *h) { return !h->run_bytes.empty(); }

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
    if (h->spilling) {
        set_error("smi_bamsort_add_segment: smi_bamsort_spill_end comes first");
        return SMI_ERR_STATE;
    }
    if (h->arena_used + bytes + kPerRecord * total > h->resident_bytes) {
        if (!h->run_mode) return sort_too_large(h);
        if (!h->arena_used) return sort_segment_too_large(h, bytes, total);
        std::memset(h->ms, 0, sizeof h->ms);
        return 3;  // full: the caller spills what the arena holds and hands the segment in again
    }
    const size_t held = (size_t)(h->n_records - h->n_spilled);  // records in the arena
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    std::memset(h->ms, 0, sizeof h->ms);
    const size_t arena_limit = (size_t)(h->resident_bytes - kPerRecord * total);
    if (int rc = sort_grow_keep(&h->d_arena, h->arena_cap, h->arena_used, h->arena_used + bytes, arena_limit, s)) return rc;
    if (int rc = sort_grow_keep(&h->d_key, h->key_cap, held, held + N, 0, s)) return rc;
    if (int rc = sort_grow_keep(&h->d_off, h->off_cap, held, held + N, 0, s)) return rc;
    if (int rc = sort_grow_keep(&h->d_len, h->len_cap, held, held + N, 0, s)) return rc;
    if (int rc = sort_grow(&h->d_recs, h->recs_cap, N)) return rc;
    h->failed = true;  // until the segment is through
    SMI_HIP(hipMemcpyAsync(h->d_arena + h->arena_used, bam + first, bytes, hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemcpyAsync(h->d_recs, recs, N * sizeof(smi_bam_record), hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemsetAsync(h->d_stop, 0xff, sizeof(unsigned long long), s));
    if (int rc = h->ev.begin(s)) return rc;
    hipLaunchKernelGGL(k_sort_key, dim3(sort_grid(N)), dim3(kSortBlock), 0, s, (const smi_bam_record *)h->d_recs, (uint32_t)n, h->n_ref, first, (uint64_t)h->arena_used,
                       h->d_key + held, h->d_off + held, h->d_len + held, h->d_stop);
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

// What finish and a spill share: the stable sort of n keys to their ordinals (iota: n ordinals of room, read by the sort alone), the
// lengths in sorted order as output offsets (ooff: n + 1 entries, the last one the total) and the windows over them, which come to
// h->win_rank and h->win_byte.  slen (may be null, may be iota): the lengths in sorted order as they are.  `total`: the bytes of the n records.
int sort_order(smi_bamsort *h, size_t n, const unsigned long long *key, unsigned long long *skey, uint32_t *iota, uint32_t *ord, const uint32_t *len,
               uint32_t *slen, uint64_t *ooff, uint64_t total, float *ms) {
    hipStream_t s = h->ctx->stream;
    // at most 2 * total / window_bytes + 1 windows (K-SORT-WINDOWS), and no more than records
    const size_t cap_w = (size_t)std::min<uint64_t>(n, 2 * total / h->window_bytes + 2);
    DevBuf<uint32_t> wrank("BamSort"), nwin("BamSort");
    DevBuf<uint64_t> wbyte("BamSort");
    Scratch cub("BamSort");
    if (int rc = wrank.alloc(cap_w + 1)) return rc;
    if (int rc = wbyte.alloc(cap_w + 1)) return rc;
    if (int rc = nwin.alloc(1)) return rc;
    int ref_bits = 1;  // the ranks 0 .. n_ref
    while (ref_bits < 31 && (1ll << ref_bits) <= h->n_ref) ref_bits++;
    const auto sort = [&](void *p, size_t &t) { return hipcub::DeviceRadixSort::SortPairs(p, t, key, skey, iota, ord, (int)n, 0, 33 + ref_bits, s); };
    const auto offsets = [&](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, ooff, ooff, (int)(n + 1), s); };
    if (int rc = reserve(cub, sort, offsets)) return rc;
    if (int rc = h->ev.begin(s)) return rc;
    hipLaunchKernelGGL(k_sort_iota, dim3(sort_grid(n)), dim3(kSortBlock), 0, s, iota, (uint32_t)n);
    SMI_HIP(hipGetLastError());
    if (int rc = run_reserved(cub, sort)) return rc;
    hipLaunchKernelGGL(k_sort_perm, dim3(sort_grid(n + 1)), dim3(kSortBlock), 0, s, (const uint32_t *)ord, len, (uint32_t)n, ooff);
    SMI_HIP(hipGetLastError());
    if (slen) {
        hipLaunchKernelGGL(k_run_len, dim3(sort_grid(n)), dim3(kSortBlock), 0, s, (const uint32_t *)ord, len, (uint32_t)n, slen);
        SMI_HIP(hipGetLastError());
    }
    if (int rc = run_reserved(cub, offsets)) return rc;
    hipLaunchKernelGGL(k_sort_windows, dim3(1), dim3(1), 0, s, (const uint64_t *)ooff, (uint32_t)n, h->window_bytes, (uint32_t)cap_w, wrank.p, wbyte.p, nwin.p);
    SMI_HIP(hipGetLastError());
    if (int rc = h->ev.end(s, ms)) return rc;
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
    if (h->win_rank[nw] != n || h->win_byte[nw] != total) {  // (cannot happen: the lengths sum to the bytes taken)
        set_error("BamSort: the windows do not add up to the records taken");
        return SMI_ERR_STATE;
    }
    return SMI_OK;
}

uint64_t sort_largest_window(const smi_bamsort *h) {
    uint64_t largest = 0;
    for (size_t k = 0; k + 1 < h->win_byte.size(); k++) largest = std::max(largest, h->win_byte[k + 1] - h->win_byte[k]);
    return largest;
}

// the window buffer: room for `bytes` and the deflater's reach of 256 bytes behind them
int sort_window_buffer(smi_bamsort *h, uint64_t bytes) {
    if (h->d_win && bytes <= h->win_cap) return SMI_OK;
    if (int rc = sort_drop(&h->d_win, &h->win_cap)) return rc;
    SMI_HIP(hipMalloc((void **)&h->d_win, (size_t)bytes + 256));
    h->win_cap = (size_t)bytes;
    return SMI_OK;
}

int sort_finish(smi_bamsort *h) {
    SMI_HIP(hipSetDevice(h->ctx->device));
    const size_t n = (size_t)h->n_records;
    std::memset(h->ms, 0, sizeof h->ms);
    h->win_rank.assign(1, 0);
    h->win_byte.assign(1, 0);
    if (!n) return SMI_OK;
    {
        DevBuf<unsigned long long> skey("BamSort");
        DevBuf<uint32_t> iota("BamSort");
        if (int rc = skey.alloc(n)) return rc;
        if (int rc = iota.alloc(n)) return rc;
        SMI_HIP(hipMalloc((void **)&h->d_ord, n * sizeof(uint32_t)));
        SMI_HIP(hipMalloc((void **)&h->d_ooff, (n + 1) * sizeof(uint64_t)));
        if (int rc = sort_order(h, n, h->d_key, skey.p, iota.p, h->d_ord, h->d_len, nullptr, h->d_ooff, h->arena_used, &h->ms[SMI_BAMSORT_MS_SORT])) return rc;
    }
    // the keys have done their work
    if (int rc = sort_drop(&h->d_key, &h->key_cap)) return rc;
    const uint64_t largest = sort_largest_window(h);
    if (int rc = sort_window_buffer(h, largest)) return rc;
    h->counts[SMI_BAMSORT_WINDOWS] = (int64_t)h->win_rank.size() - 1;
    h->counts[SMI_BAMSORT_LARGEST_WINDOW] = (int64_t)largest;
    return SMI_OK;
}

// finish over runs: the global order of the runs' keys, the windows, and the slice every window draws from every run
int sort_finish_runs(smi_bamsort *h) {
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    const size_t n = (size_t)h->n_records, runs = h->run_bytes.size();
    if (h->spilling || h->n_spilled != h->n_records) {
        set_error("smi_bamsort_finish: runs were written, so what the arena holds is spilled first (smi_bamsort_spill_begin .. smi_bamsort_spill_end)");
        return SMI_ERR_STATE;
    }
    std::memset(h->ms, 0, sizeof h->ms);
    // the arena and what described it are gone: staging buffer and window buffer take its place
    if (int rc = sort_drop(&h->d_arena, &h->arena_cap)) return rc;
    if (int rc = sort_drop(&h->d_key, &h->key_cap)) return rc;
    if (int rc = sort_drop(&h->d_off, &h->off_cap)) return rc;
    if (int rc = sort_drop(&h->d_len, &h->len_cap)) return rc;
    if (int rc = sort_drop(&h->d_recs, &h->recs_cap)) return rc;
    if (int rc = sort_drop(&h->d_win, &h->win_cap)) return rc;
    if (int rc = sort_drop(&h->d_ord)) return rc;
    {
        DevBuf<unsigned long long> skey("BamSort");
        DevBuf<uint32_t> iota("BamSort");
        if (int rc = skey.alloc(n)) return rc;
        if (int rc = iota.alloc(n)) return rc;
        SMI_HIP(hipMalloc((void **)&h->d_ord, n * sizeof(uint32_t)));
        SMI_HIP(hipMalloc((void **)&h->d_ooff, (n + 1) * sizeof(uint64_t)));
        if (int rc = sort_order(h, n, h->d_rkey, skey.p, iota.p, h->d_ord, h->d_rlen, nullptr, h->d_ooff, h->spilled_bytes, &h->ms[SMI_BAMSORT_MS_MERGE_SORT]))
            return rc;
    }
    // the sorted keys, the iota, the runs' keys and their lengths are freed before rank_of (4 bytes per record) is allocated
    if (int rc = sort_drop(&h->d_rkey, &h->rkey_cap)) return rc;
    if (int rc = sort_drop(&h->d_rlen, &h->rlen_cap)) return rc;
    const size_t borders = h->win_rank.size(), entries = borders * runs;
    {
        DevBuf<uint32_t> rank_of("BamSort"), wrank("BamSort"), sord("BamSort");
        DevBuf<uint64_t> rbytes("BamSort"), sbyte("BamSort");
        if (int rc = rank_of.alloc(n)) return rc;
        if (int rc = wrank.put(h->win_rank, s)) return rc;
        if (int rc = rbytes.put(h->run_bytes, s)) return rc;
        if (int rc = sord.alloc(entries)) return rc;
        if (int rc = sbyte.alloc(entries)) return rc;
        SMI_HIP(hipMalloc((void **)&h->d_run_first, (runs + 1) * sizeof(uint32_t)));
        SMI_HIP(hipMemcpyAsync(h->d_run_first, h->run_first.data(), (runs + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if (int rc = h->ev.begin(s)) return rc;
        hipLaunchKernelGGL(k_merge_rank, dim3(sort_grid(n)), dim3(kSortBlock), 0, s, (const uint32_t *)h->d_ord, (uint32_t)n, rank_of.p);
        SMI_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_merge_slices, dim3(sort_grid(entries)), dim3(kSortBlock), 0, s, (const uint32_t *)rank_of.p, (const uint64_t *)h->d_roff,
                           (const uint32_t *)h->d_run_first, (const uint64_t *)rbytes.p, (const uint32_t *)wrank.p, (uint64_t)entries, (uint32_t)runs, sord.p, sbyte.p);
        SMI_HIP(hipGetLastError());
        if (int rc = h->ev.end(s, &h->ms[SMI_BAMSORT_MS_SLICES])) return rc;
        h->slice_ord.resize(entries);
        h->slice_byte.resize(entries);
        SMI_HIP(hipMemcpy(h->slice_ord.data(), sord.p, entries * sizeof(uint32_t), hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(h->slice_byte.data(), sbyte.p, entries * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    // every window's slices begin where the window before left each run, and add up to the window
    for (size_t k = 0; k + 1 < borders; k++) {
        uint64_t sum = 0;
        bool ok = true;
        for (size_t j = 0; j < runs; j++) {
            const uint64_t a = h->slice_byte[k * runs + j], b = h->slice_byte[(k + 1) * runs + j];
            ok = ok && a <= b && b <= h->run_bytes[j] && (k || !a) && (k + 2 < borders || b == h->run_bytes[j]);
            sum += b - a;
        }
        if (!ok || sum != h->win_byte[k + 1] - h->win_byte[k]) {  // (cannot happen)
            set_error("BamSort: the slices of window " + std::to_string(k) + " do not add up to it");
            return SMI_ERR_STATE;
        }
    }
    const uint64_t largest = sort_largest_window(h);
    if (int rc = sort_window_buffer(h, largest)) return rc;
    SMI_HIP(hipMalloc((void **)&h->d_stage, (size_t)std::max<uint64_t>(largest, 1)));
    SMI_HIP(hipMalloc((void **)&h->d_delta, runs * sizeof(int64_t)));
    h->delta.resize(runs);
    h->counts[SMI_BAMSORT_WINDOWS] = (int64_t)borders - 1;
    h->counts[SMI_BAMSORT_LARGEST_WINDOW] = (int64_t)largest;
    return SMI_OK;
}

// the deflated window buffer to the caller: what smi_bamsort_window and smi_bamsort_merge_window share behind their gathers
int sort_emit(smi_bamsort *h, size_t bytes, uint8_t *out_bgzf, size_t cap, size_t *n_out, uint8_t *out_inflated, const char *who) {
    hipStream_t s = h->ctx->stream;
    if (int rc = h->ev.begin(s)) return rc;
    size_t z = 0;
    if (int rc = smi_bgzf_deflate_device(h->ctx, h->d_win, bytes, out_bgzf, cap, &z)) return rc;
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMSORT_MS_DEFLATE])) return rc;
    if (z < 28) {  // (cannot happen: the deflater closes its stream with the end-of-file block)
        set_error(std::string(who) + ": the deflater wrote no end-of-file block");
        return SMI_ERR_STATE;
    }
    *n_out = z - 28;  // the caller ends the file
    if (out_inflated) SMI_HIP(hipMemcpy(out_inflated, h->d_win, bytes, hipMemcpyDeviceToHost));
    h->counts[SMI_BAMSORT_BYTES_OUT] += (int64_t)bytes;
    return SMI_OK;
}

int sort_window_state(const smi_bamsort *h, int64_t k, const char *who) {
    if (h->failed || !h->finished) {
        set_error(std::string(who) + (h->failed ? ": an earlier call failed" : ": smi_bamsort_finish comes first"));
        return SMI_ERR_STATE;
    }
    if (k < 0 || (size_t)k + 1 >= h->win_rank.size()) {
        set_error(std::string(who) + ": no window " + std::to_string(k));
        return SMI_ERR_INVALID;
    }
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
        if (int rc = sort_merging(h) ? sort_finish_runs(h) : sort_finish(h)) {
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
    if (int rc = sort_window_state(h, k, "smi_bamsort_window")) return rc;
    if (sort_merging(h)) {
        set_error("smi_bamsort_window: the records are in run files; smi_bamsort_merge_window takes their slices");
        return SMI_ERR_STATE;
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
    if (int rc = sort_gather(h, (size_t)k, h->d_ooff)) return rc;
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMSORT_MS_GATHER])) return rc;
    return sort_emit(h, bytes, out_bgzf, cap, n_out, out_inflated, "smi_bamsort_window");
}

extern "C" int smi_bamsort_run_mode(smi_bamsort *h) {
    if (!h) {
        set_error("smi_bamsort_run_mode: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->n_records || h->failed || h->finished) {
        set_error("smi_bamsort_run_mode: comes before the first segment");
        return SMI_ERR_STATE;
    }
    h->run_mode = true;
    return SMI_OK;
}

extern "C" int smi_bamsort_spill_begin(smi_bamsort *h, int64_t *n_windows, int64_t *n_records, uint64_t *n_bytes) {
    if (!h || !n_windows || !n_records || !n_bytes) {
        set_error("smi_bamsort_spill_begin: null argument");
        return SMI_ERR_INVALID;
    }
    if (!h->run_mode || h->failed || h->finished || h->spilling || h->n_records == h->n_spilled) {
        set_error(!h->run_mode ? "smi_bamsort_spill_begin: smi_bamsort_run_mode comes first"
                  : h->failed  ? "smi_bamsort_spill_begin: an earlier call failed"
                               : "smi_bamsort_spill_begin: nothing to spill, a spill is open or the sort is finished");
        return SMI_ERR_STATE;
    }
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    const size_t done = (size_t)h->n_spilled, n = (size_t)(h->n_records - h->n_spilled);
    std::memset(h->ms, 0, sizeof h->ms);
    h->failed = true;  // until the run is ordered
    if (int rc = sort_grow_keep(&h->d_rkey, h->rkey_cap, done, done + n, 0, s)) return rc;
    if (int rc = sort_grow_keep(&h->d_rlen, h->rlen_cap, done, done + n, 0, s)) return rc;
    if (int rc = sort_grow_keep(&h->d_roff, h->roff_cap, done, done + n + 1, 0, s)) return rc;
    if (int rc = sort_drop(&h->d_ord)) return rc;
    SMI_HIP(hipMalloc((void **)&h->d_ord, n * sizeof(uint32_t)));
    // the run's sorted keys, lengths and run-file offsets are written where they stay; the lengths' place serves as the sort's iota first
    if (int rc = sort_order(h, n, h->d_key, h->d_rkey + done, h->d_rlen + done, h->d_ord, h->d_len, h->d_rlen + done, h->d_roff + done, h->arena_used,
                            &h->ms[SMI_BAMSORT_MS_SORT]))
        return rc;
    if (int rc = sort_window_buffer(h, sort_largest_window(h))) return rc;
    h->failed = false;
    h->spilling = true;
    *n_windows = (int64_t)h->win_rank.size() - 1;
    *n_records = (int64_t)n;
    *n_bytes = h->arena_used;
    return SMI_OK;
}

extern "C" int smi_bamsort_spill_window(smi_bamsort *h, int64_t k, uint8_t *out, size_t cap, size_t *n_out) {
    if (!h || !n_out) {
        set_error("smi_bamsort_spill_window: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed || !h->spilling) {
        set_error(h->failed ? "smi_bamsort_spill_window: an earlier call failed" : "smi_bamsort_spill_window: smi_bamsort_spill_begin comes first");
        return SMI_ERR_STATE;
    }
    if (k < 0 || (size_t)k + 1 >= h->win_rank.size()) {
        set_error("smi_bamsort_spill_window: no window " + std::to_string(k));
        return SMI_ERR_INVALID;
    }
    const size_t bytes = (size_t)(h->win_byte[k + 1] - h->win_byte[k]);
    *n_out = bytes;
    if (!out) return SMI_OK;
    if (cap < bytes) return 1;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    std::memset(h->ms, 0, sizeof h->ms);
    if (int rc = h->ev.begin(s)) return rc;
    if (int rc = sort_gather(h, (size_t)k, h->d_roff + h->n_spilled)) return rc;
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMSORT_MS_SPILL_GATHER])) return rc;
    SMI_HIP(hipMemcpy(out, h->d_win, bytes, hipMemcpyDeviceToHost));
    return SMI_OK;
}

extern "C" int smi_bamsort_spill_end(smi_bamsort *h) {
    if (!h) {
        set_error("smi_bamsort_spill_end: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed || !h->spilling) {
        set_error(h->failed ? "smi_bamsort_spill_end: an earlier call failed" : "smi_bamsort_spill_end: smi_bamsort_spill_begin comes first");
        return SMI_ERR_STATE;
    }
    SMI_HIP(hipSetDevice(h->ctx->device));
    SMI_HIP(hipStreamSynchronize(h->ctx->stream));
    std::memset(h->ms, 0, sizeof h->ms);
    if (int rc = sort_drop(&h->d_ord)) return rc;
    if (h->run_first.empty()) h->run_first.push_back(0);
    h->run_first.push_back((uint32_t)h->n_records);
    h->run_bytes.push_back(h->arena_used);
    h->spilled_bytes += h->arena_used;
    h->counts[SMI_BAMSORT_RUNS] = (int64_t)h->run_bytes.size();
    h->counts[SMI_BAMSORT_RUN_BYTES] = (int64_t)h->spilled_bytes;
    h->counts[SMI_BAMSORT_LARGEST_RUN] = std::max<int64_t>(h->counts[SMI_BAMSORT_LARGEST_RUN], (int64_t)h->arena_used);
    h->n_spilled = h->n_records;
    h->arena_used = 0;
    h->counts[SMI_BAMSORT_ARENA_BYTES] = 0;
    h->spilling = false;
    return SMI_OK;
}

extern "C" int smi_bamsort_window_slices(const smi_bamsort *h, int64_t k, int64_t *n_runs, uint64_t *first_byte, uint64_t *n_bytes, uint32_t *first_ordinal,
                                         size_t cap) {
    if (!h || !n_runs) {
        set_error("smi_bamsort_window_slices: null argument");
        return SMI_ERR_INVALID;
    }
    if (int rc = sort_window_state(h, k, "smi_bamsort_window_slices")) return rc;
    const size_t runs = h->run_bytes.size();
    *n_runs = (int64_t)runs;
    if (!first_byte || !n_bytes) return SMI_OK;
    if (cap < runs) return 1;
    for (size_t j = 0; j < runs; j++) {
        first_byte[j] = h->slice_byte[(size_t)k * runs + j];
        n_bytes[j] = h->slice_byte[((size_t)k + 1) * runs + j] - first_byte[j];
        if (first_ordinal) first_ordinal[j] = h->slice_ord[(size_t)k * runs + j];
    }
    return SMI_OK;
}

extern "C" int smi_bamsort_merge_window(smi_bamsort *h, int64_t k, const uint8_t *slices, size_t n_slices, uint8_t *out_bgzf, size_t cap, size_t *n_out,
                                        uint8_t *out_inflated, size_t cap_inflated, size_t *n_inflated) {
    if (!h || !n_out || !n_inflated) {
        set_error("smi_bamsort_merge_window: null argument");
        return SMI_ERR_INVALID;
    }
    if (int rc = sort_window_state(h, k, "smi_bamsort_merge_window")) return rc;
    if (!sort_merging(h)) {
        set_error("smi_bamsort_merge_window: no run was written; smi_bamsort_window gathers from the arena");
        return SMI_ERR_STATE;
    }
    const size_t bytes = (size_t)(h->win_byte[k + 1] - h->win_byte[k]), runs = h->run_bytes.size();
    size_t bound = 0;
    if (int rc = smi_bgzf_deflate_device(h->ctx, h->d_win, bytes, nullptr, 0, &bound)) return rc;
    *n_out = bound;
    *n_inflated = bytes;
    if (!out_bgzf) return SMI_OK;
    if (cap < bound || (out_inflated && cap_inflated < bytes)) return 1;
    if (!slices || n_slices != bytes) {
        set_error("smi_bamsort_merge_window: window " + std::to_string(k) + " takes the " + std::to_string(bytes) + " bytes of its slices, run after run");
        return SMI_ERR_INVALID;
    }
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    std::memset(h->ms, 0, sizeof h->ms);
    uint64_t at = 0;  // where run j's slice begins in the staging buffer, minus where it begins in the run file
    for (size_t j = 0; j < runs; j++) {
        h->delta[j] = (int64_t)at - (int64_t)h->slice_byte[(size_t)k * runs + j];
        at += h->slice_byte[((size_t)k + 1) * runs + j] - h->slice_byte[(size_t)k * runs + j];
    }
    if (int rc = h->ev.begin(s)) return rc;
    SMI_HIP(hipMemcpyAsync(h->d_stage, slices, bytes, hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemcpyAsync(h->d_delta, h->delta.data(), runs * sizeof(int64_t), hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemsetAsync(h->d_stop, 0xff, sizeof(unsigned long long), s));
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMSORT_MS_STAGE_UPLOAD])) return rc;
    const uint32_t r0 = h->win_rank[k], n = h->win_rank[k + 1] - r0;
    if (int rc = h->ev.begin(s)) return rc;
    hipLaunchKernelGGL(k_merge_gather<16>, dim3(sort_grid(n, kSortRecs)), dim3(kSortBlock), 0, s, (const uint8_t *)h->d_stage, (uint64_t)bytes,
                       (const uint64_t *)h->d_roff, (const uint32_t *)h->d_ord, (const uint64_t *)h->d_ooff, (const uint32_t *)h->d_run_first, (uint32_t)runs,
                       (const int64_t *)h->d_delta, r0, n, h->win_byte[k], h->d_win, h->d_stop);
    SMI_HIP(hipGetLastError());
    if (int rc = h->ev.end(s, &h->ms[SMI_BAMSORT_MS_GATHER])) return rc;
    unsigned long long bad = kNoRecord;
    SMI_HIP(hipMemcpy(&bad, h->d_stop, sizeof bad, hipMemcpyDeviceToHost));
    if (bad != kNoRecord) {  // (cannot happen: the slices are the windows' own)
        h->failed = true;
        set_error("smi_bamsort_merge_window: the record of rank " + std::to_string(bad) + " lies outside the slices of window " + std::to_string(k));
        return SMI_ERR_STATE;
    }
    return sort_emit(h, bytes, out_bgzf, cap, n_out, out_inflated, "smi_bamsort_merge_window");
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
    if (h->run_mode) {
        set_error("smi_bamsort_host_loop: the host loop needs the arena, which run mode does not keep");
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
        if (int rc = sort_gather(h, k, h->d_ooff)) return rc;
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
