// smi_bamindex.hip -- `BamIndex`: the .bai (SAM specification 5.2) of a coordinate-sorted BAM, in the place of `samtools index`.  The file is
// this build's own canonical form, defined in DESIGN.md section 8l; tests/baimodel.py restates that definition.
//
// The caller hands in the file's BGZF blocks in file order (smi_bamindex_add_blocks) and the inflated stream in segments with their record
// index (smi_bamindex_add_segment).  Per segment, K-BAI:
//   K-BAI-REC    kBaiLanes lanes per record: the reference length of the stored CIGAR summed by the lanes (sub-wave shuffle reduction, as
//                K-SNP sums it), then one lane: extent, bin (reg2bin), first and last window and the two virtual offsets, each by a binary
//                search of the stream offset in the segment's slice of the block table; the records the run stops at (atomicMin)
//   K-BAI-ORDER  one lane per record: the order check against the record in front (the last key of the segment before is carried), the head
//                flags where (ref_id, bin) changes, the per-reference offsets and counts (one atomic per wave where the wave's records lie
//                on one reference); hipcub inclusive scan of the head flags
//   K-BAI-CHUNK  compaction: a head writes its chunk's key and start, the last record of a run its end, behind the chunks of the segments
//                before; a run that goes on across the border writes the end of the chunk that is already there
//   K-BAI-LIN    kBaiLanes lanes per record share its window loop: 64-bit atomicMin of the record's offset into every window it covers
// and at smi_bamindex_finish: one stable hipcub radix sort of the chunks by (ref_id, bin), a run-length encode for the chunks per bin,
// K-BAI-BINS for the bins per reference, K-BAI-FILL (one block per reference: the forward fill of the empty windows as a running maximum,
// the window values of a sorted file being non-decreasing).  The host serialises the sorted arrays.
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "smi_device.h"
#include "smi_handle.h"
#include "smi_internal.h"

namespace smi {
namespace {

constexpr int kBaiBlock = 256;
constexpr int kBaiLanes = 16;  // lanes per record of K-BAI-REC and K-BAI-LIN (why 16)
constexpr int kBaiRecs = kBaiBlock / kBaiLanes;
constexpr unsigned long long kNoRecord = ~0ull;
constexpr int64_t kMaxEnd = 1ll << 29;  // the last position the five bin levels and the 16 kb windows hold
constexpr uint32_t kMaxWindows = 1u << 15;
constexpr uint32_t kMetaBin = 37450;
constexpr uint32_t kNoBin = 0xffffffffu;

enum : uint32_t { BAI_PLACED = 1, BAI_FLAG4 = 2, BAI_KIND_SHIFT = 8 };
enum : uint32_t { STOP_NEG_POS = 1, STOP_TOO_FAR = 2, STOP_REF = 3, STOP_PAST_REF = 4, STOP_ORDER = 5 };
enum { W_ERR = 0, W_NO_COOR, W_COUNT };

struct BaiRec {
    uint64_t vbeg, vend;
    int32_t ref, beg, end;  // end: exclusive; at most 2^29 where BAI_PLACED is set
    uint32_t bin, flags, pad;
};
struct Voff {
    uint64_t beg, end;
};
struct Carry {  // the last record of the segment before
    int32_t has_prev, ref, pos;
    uint32_t bin;
};
struct Meta {  // per reference
    unsigned long long *min_off, *max_off, *n_mapped, *n_flag4;
    uint32_t *max_end, *n_bin;
};

// start[0] <= p: the last block j with start[j] <= p (the slice ends with the entry of the position behind its last byte)
__device__ __forceinline__ uint64_t virtual_offset(const uint64_t *__restrict__ start, const uint64_t *__restrict__ coff, uint32_t nb, uint64_t p) {
    uint32_t lo = 0, hi = nb;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (start[mid] <= p) lo = mid;
        else hi = mid;
    }
    return coff[lo] << 16 | ((p - start[lo]) & 0xffffu);
}

__device__ __forceinline__ uint32_t reg2bin(uint32_t beg, uint32_t end) {
    const uint32_t e = end - 1;
    if (beg >> 14 == e >> 14) return 4681 + (beg >> 14);
    if (beg >> 17 == e >> 17) return 585 + (beg >> 17);
    if (beg >> 20 == e >> 20) return 73 + (beg >> 20);
    if (beg >> 23 == e >> 23) return 9 + (beg >> 23);
    if (beg >> 26 == e >> 26) return 1 + (beg >> 26);
    return 0;
}

struct RecArgs {
    const uint8_t *bam;
    const smi_bam_record *recs;
    uint32_t n;
    int32_t n_ref;
    uint64_t stream_off;
    const uint64_t *blk_start, *blk_coff;
    uint32_t n_blk;
    const uint32_t *win_cap;
    BaiRec *out;
    unsigned long long *words;
};

__global__ __launch_bounds__(kBaiBlock) void k_bai_rec(RecArgs a) {
    const uint32_t i = blockIdx.x * kBaiRecs + (threadIdx.x / kBaiLanes), sub = threadIdx.x % kBaiLanes;
    const bool valid = i < a.n;
    unsigned long long sum = 0;
    uint64_t cigar = 0, rec_off = 0;
    uint32_t n_cigar = 0, rec_len = 0, flag = 0;
    int32_t ref = -1, pos = 0;
    if (valid) {
        const smi_bam_record *r = a.recs + i;
        cigar = r->cigar_off;
        n_cigar = r->n_cigar;
        rec_off = r->rec_off;
        rec_len = r->rec_len;
        flag = r->flag;
        ref = r->ref_id;
        pos = r->pos;
        for (uint32_t k = sub; k < n_cigar; k += kBaiLanes) {
            const uint32_t w = ld_u32(a.bam + cigar + 4ull * k);
            if ((0x18Du >> (w & 15)) & 1) sum += w >> 4;  // M D N = X
        }
    }
#pragma unroll
    for (int m = kBaiLanes / 2; m; m >>= 1) sum += __shfl_xor(sum, m, kBaiLanes);
    if (!valid || sub) return;
    BaiRec o = {};
    o.ref = ref;
    o.beg = pos;
    o.bin = kNoBin;
    o.vbeg = virtual_offset(a.blk_start, a.blk_coff, a.n_blk, a.stream_off + rec_off);
    o.vend = virtual_offset(a.blk_start, a.blk_coff, a.n_blk, a.stream_off + rec_off + rec_len);
    if (flag & 4) o.flags |= BAI_FLAG4;
    if (ref >= 0) {
        const unsigned long long len = (flag & 4) || !n_cigar || !sum ? 1ull : sum;
        const unsigned long long end = (unsigned long long)(pos < 0 ? 0 : pos) + len;
        uint32_t stop = 0;
        if (pos < 0) stop = STOP_NEG_POS;
        else if (end > (unsigned long long)kMaxEnd) stop = STOP_TOO_FAR;
        else if (ref >= a.n_ref) stop = STOP_REF;
        else if ((end - 1) >> 14 >= a.win_cap[ref]) stop = STOP_PAST_REF;
        if (stop) {
            o.flags |= stop << BAI_KIND_SHIFT;
            o.end = pos;
            atomicMin(a.words + W_ERR, (unsigned long long)i);
        } else {
            o.end = (int32_t)end;
            o.bin = reg2bin((uint32_t)pos, (uint32_t)end);
            o.flags |= BAI_PLACED;
        }
    }
    a.out[i] = o;
}

__device__ __forceinline__ unsigned long long order_key(int32_t ref, int32_t pos) {
    return ref < 0 ? ~0ull : (unsigned long long)(uint32_t)ref << 32 | (uint32_t)pos;
}

__global__ __launch_bounds__(kBaiBlock) void k_bai_order(BaiRec *__restrict__ rec, uint32_t n, const Carry *__restrict__ carry, uint32_t *__restrict__ head,
                                                         Meta m, unsigned long long *__restrict__ words) {
    const uint32_t i = blockIdx.x * kBaiBlock + threadIdx.x;
    const bool valid = i < n;
    int32_t ref = -1;
    bool placed = false, flag4 = false, unplaced = false;
    unsigned long long vbeg = ~0ull, vend = 0;
    uint32_t end = 0;
    if (valid) {
        const BaiRec c = rec[i];
        unplaced = c.ref < 0;
        Carry p;
        if (i) {
            const BaiRec *q = rec + (i - 1);
            p.has_prev = 1;
            p.ref = q->ref;
            p.pos = q->beg;
            p.bin = q->bin;
        } else
            p = *carry;
        placed = c.flags & BAI_PLACED;
        flag4 = c.flags & BAI_FLAG4;
        if (p.has_prev && order_key(c.ref, c.beg) < order_key(p.ref, p.pos) && !(c.flags >> BAI_KIND_SHIFT)) {
            rec[i].flags = c.flags | STOP_ORDER << BAI_KIND_SHIFT;
            atomicMin(words + W_ERR, (unsigned long long)i);
        }
        head[i] = placed && !(p.has_prev && p.ref == c.ref && p.bin == c.bin);
        if (placed) {
            ref = c.ref;
            vbeg = c.vbeg;
            vend = c.vend;
            end = (uint32_t)c.end;
        }
    }
    const unsigned long long no_coor = __ballot(unplaced);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && no_coor) atomicAdd(words + W_NO_COOR, (unsigned long long)__popcll(no_coor));
    // the per-reference values: one set of atomics per wave where all its records lie on one reference
    const int32_t ref0 = __shfl(ref, 0);
    if (__all(ref == ref0)) {
        if (ref0 < 0) return;
        const unsigned long long mapped = __ballot(placed && !flag4), unm = __ballot(placed && flag4);
#pragma unroll
        for (int s = 32; s; s >>= 1) {
            const unsigned long long b = __shfl_xor(vbeg, s), e = __shfl_xor(vend, s);
            const uint32_t x = __shfl_xor(end, s);
            vbeg = b < vbeg ? b : vbeg;
            vend = e > vend ? e : vend;
            end = x > end ? x : end;
        }
        if (lane == 0) {
            atomicMin(m.min_off + ref0, vbeg);
            atomicMax(m.max_off + ref0, vend);
            atomicMax(m.max_end + ref0, end);
            if (mapped) atomicAdd(m.n_mapped + ref0, (unsigned long long)__popcll(mapped));
            if (unm) atomicAdd(m.n_flag4 + ref0, (unsigned long long)__popcll(unm));
        }
    } else if (placed) {
        atomicMin(m.min_off + ref, vbeg);
        atomicMax(m.max_off + ref, vend);
        atomicMax(m.max_end + ref, end);
        atomicAdd(flag4 ? m.n_flag4 + ref : m.n_mapped + ref, 1ull);
    }
}

__global__ __launch_bounds__(kBaiBlock) void k_bai_chunk(const BaiRec *__restrict__ rec, uint32_t n, const uint32_t *__restrict__ head,
                                                         const uint32_t *__restrict__ incl, uint64_t base, uint64_t cap, unsigned long long *__restrict__ ckey,
                                                         Voff *__restrict__ cval, Carry *__restrict__ carry) {
    const uint32_t i = blockIdx.x * kBaiBlock + threadIdx.x;
    if (i >= n) return;
    const BaiRec c = rec[i];
    if (i == n - 1) {
        Carry k = {1, c.ref, c.beg, c.bin};
        *carry = k;
    }
    if (!(c.flags & BAI_PLACED)) return;
    const uint64_t idx = base + incl[i] - 1;
    if (idx >= cap) return;  // (cannot happen: the chunk arrays hold base + n entries, and a record that is no head has a chunk in front)
    if (head[i]) {
        ckey[idx] = (unsigned long long)(uint32_t)c.ref << 32 | c.bin;
        cval[idx].beg = c.vbeg;
    }
    bool tail = i == n - 1;
    if (!tail) {
        const BaiRec *q = rec + (i + 1);
        tail = !((q->flags & BAI_PLACED) && q->ref == c.ref && q->bin == c.bin);
    }
    if (tail) cval[idx].end = c.vend;
}

__global__ __launch_bounds__(kBaiBlock) void k_bai_lin(const BaiRec *__restrict__ rec, uint32_t n, const uint64_t *__restrict__ win_off,
                                                       unsigned long long *__restrict__ lin) {
    const uint32_t i = blockIdx.x * kBaiRecs + (threadIdx.x / kBaiLanes), sub = threadIdx.x % kBaiLanes;
    if (i >= n) return;
    const BaiRec *c = rec + i;
    if (!(c->flags & BAI_PLACED)) return;
    const uint32_t wb = (uint32_t)c->beg >> 14, we = ((uint32_t)c->end - 1) >> 14;
    const unsigned long long v = c->vbeg;
    unsigned long long *w0 = lin + win_off[c->ref];
    for (uint32_t w = wb + sub; w <= we; w += kBaiLanes) atomicMin(w0 + w, v);
}

// the end offset the last record of a segment took for the position behind the known blocks, once the next block shows another one
__global__ void k_bai_patch(Voff *cval, long long chunk, unsigned long long *max_off, int32_t ref, unsigned long long v) {
    if (chunk >= 0) cval[chunk].end = v;
    if (ref >= 0) atomicMax(max_off + ref, v);
}

__global__ __launch_bounds__(kBaiBlock) void k_bai_bins(const unsigned long long *__restrict__ ukey, const uint32_t *__restrict__ n_runs, uint32_t *__restrict__ n_bin) {
    const uint32_t j = blockIdx.x * kBaiBlock + threadIdx.x;
    if (j < *n_runs) atomicAdd(n_bin + (uint32_t)(ukey[j] >> 32), 1u);
}

// K-BAI-FILL: block r fills the windows of reference r: an empty window takes the value in front of it, leading ones 0
__global__ __launch_bounds__(kBaiBlock) void k_bai_fill(unsigned long long *__restrict__ lin, const uint64_t *__restrict__ win_off, const uint32_t *__restrict__ max_end) {
    using Scan = hipcub::BlockScan<unsigned long long, kBaiBlock>;
    __shared__ typename Scan::TempStorage tmp;
    __shared__ unsigned long long carry;
    const uint32_t r = blockIdx.x, e = max_end[r], n_intv = e ? ((e - 1) >> 14) + 1 : 0;
    unsigned long long *w0 = lin + win_off[r];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t t = 0; t < n_intv; t += kBaiBlock) {
        const uint32_t w = t + threadIdx.x;
        unsigned long long v = w < n_intv ? w0[w] : 0;
        if (v == ~0ull) v = 0;
        unsigned long long out;
        Scan(tmp).InclusiveScan(v, out, hipcub::Max());
        const unsigned long long c = carry;
        out = out > c ? out : c;
        if (w < n_intv) w0[w] = out;
        __syncthreads();
        if (threadIdx.x == kBaiBlock - 1) carry = out;
        __syncthreads();
    }
}

template <class T>
int grow(T **p, size_t &cap, size_t want) {
    if (want <= cap && *p) return SMI_OK;
    const size_t n = std::max<size_t>(want + want / 4, 1024);
    if (*p) SMI_HIP(hipFree(*p));
    *p = nullptr;
    cap = 0;
    SMI_HIP(hipMalloc((void **)p, n * sizeof(T)));
    cap = n;
    return SMI_OK;
}

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

inline unsigned grid(size_t n, unsigned per = kBaiBlock) { return (unsigned)std::max<size_t>(1, (n + per - 1) / per); }

const char *const kStopText[6] = {
    "",
    "it lies on a reference and its position is negative",
    "it ends behind position 2^29: BAI cannot hold the position (bins and windows end there)",
    "its ref_id is not one of the header's references",
    "it ends behind the length the header gives its reference",
    "it is out of coordinate order: records on a reference by (ref_id, pos), records without one last",
};

}  // namespace
}  // namespace smi

using namespace smi;

struct smi_bamindex {
    smi_ctx *ctx = nullptr;
    int32_t n_ref = 0;
    // the file's non-empty blocks so far: first inflated byte, coffset; after_coff: the coffset behind the last of them
    std::vector<uint64_t> blk_start, blk_coff;
    uint64_t stream_total = 0, next_coff = 0, after_coff = 0;
    // the last record of the last segment ended at the end of the known blocks and took after_coff << 16 for the position behind it
    bool pending = false;
    int64_t pending_chunk = -1;
    int32_t pending_ref = -1;
    // resident
    std::vector<uint64_t> win_off;  // [n_ref + 1]
    uint64_t *d_win_off = nullptr;
    uint32_t *d_win_cap = nullptr;
    unsigned long long *d_lin = nullptr, *d_meta64 = nullptr;  // d_meta64: min_off, max_off, n_mapped, n_flag4, each [n_ref]
    uint32_t *d_meta32 = nullptr;                               // max_end, n_bin
    unsigned long long *d_ckey = nullptr;
    Voff *d_cval = nullptr;
    size_t ckey_cap = 0, cval_cap = 0;
    uint64_t n_chunks = 0;
    Carry *d_carry = nullptr;
    unsigned long long *d_words = nullptr;
    // one segment (grow-only)
    uint8_t *d_bam = nullptr;
    smi_bam_record *d_recs = nullptr;
    BaiRec *d_rec = nullptr;
    uint32_t *d_head = nullptr, *d_incl = nullptr;
    uint64_t *d_blk = nullptr;  // start[nb], coff[nb]
    Scratch cub{"BamIndex"};    // hipcub's
    size_t bam_cap = 0, recs_cap = 0, rec_cap = 0, head_cap = 0, incl_cap = 0, blk_cap = 0;
    Events ev;
    int64_t counts[SMI_BAI_N_COUNT] = {};
    float ms[SMI_BAI_N_STAGE] = {};
    std::string error_read, bai;
    int64_t error_record = -1;
    bool failed = false, finished = false;

    Meta meta() const {
        const size_t n = (size_t)std::max(n_ref, 1);
        return {d_meta64, d_meta64 + n, d_meta64 + 2 * n, d_meta64 + 3 * n, d_meta32, d_meta32 + n};
    }
};

namespace {

void bai_release(smi_bamindex *h) {
    void *bufs[] = {h->d_win_off, h->d_win_cap, h->d_lin, h->d_meta64, h->d_meta32, h->d_ckey, h->d_cval, h->d_carry, h->d_words,
                    h->d_bam,     h->d_recs,    h->d_rec, h->d_head,   h->d_incl,   h->d_blk};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    delete h;
}

}  // namespace

extern "C" int smi_bamindex_create(smi_ctx *ctx, int32_t n_ref, const int32_t *ref_len, smi_bamindex **out) {
    if (!ctx || !out || n_ref < 0 || (n_ref && !ref_len)) {
        set_error("smi_bamindex_create: bad argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    SMI_HIP(hipSetDevice(ctx->device));
    smi_bamindex *h = new smi_bamindex();
    h->ctx = ctx;
    h->n_ref = n_ref;
    const size_t n = (size_t)std::max(n_ref, 1);
    // the windows of a reference: those its length in the header covers (a length of 0 or below: one), at most the 2^15 the format holds
    std::vector<uint32_t> cap(n, 1);
    h->win_off.assign(n + 1, 0);
    for (int32_t r = 0; r < n_ref; r++) {
        const int64_t len = std::max<int64_t>(ref_len[r], 1);
        cap[(size_t)r] = (uint32_t)std::min<int64_t>(((len - 1) >> 14) + 1, kMaxWindows);
    }
    for (size_t r = 0; r < n; r++) h->win_off[r + 1] = h->win_off[r] + cap[r];
    const size_t n_win = (size_t)h->win_off[n];
    hipStream_t s = ctx->stream;
    hipError_t e = hipMalloc((void **)&h->d_win_off, (n + 1) * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_win_cap, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_lin, n_win * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_meta64, 4 * n * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_meta32, 2 * n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_carry, sizeof(Carry));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_words, W_COUNT * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_win_off, h->win_off.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_win_cap, cap.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_lin, 0xff, n_win * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_meta64, 0, 4 * n * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_meta64, 0xff, n * sizeof(unsigned long long), s);  // min_off
    if (e == hipSuccess) e = hipMemsetAsync(h->d_meta32, 0, 2 * n * sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_carry, 0, sizeof(Carry), s);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_words, 0, W_COUNT * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // cap goes out of scope
    if (e != hipSuccess) {
        bai_release(h);
        return hip_fail(e, "smi_bamindex_create");
    }
    h->counts[SMI_BAI_WINDOWS_HELD] = (int64_t)n_win;
    *out = h;
    return SMI_OK;
}

extern "C" int smi_bamindex_free(smi_bamindex *h) {
    if (h) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        bai_release(h);
    }
    return SMI_OK;
}

extern "C" int smi_bamindex_counts(const smi_bamindex *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_bamindex_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof h->counts);
    return SMI_OK;
}

extern "C" int smi_bamindex_stage_ms(const smi_bamindex *h, float *ms) {
    if (!h || !ms) {
        set_error("smi_bamindex_stage_ms: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(ms, h->ms, sizeof h->ms);
    return SMI_OK;
}

extern "C" int smi_bamindex_error_read(const smi_bamindex *h, char *name, size_t cap, int64_t *record) {
    if (!h || !record || (cap && !name)) {
        set_error("smi_bamindex_error_read: null argument");
        return SMI_ERR_INVALID;
    }
    return handle::error_read(h->error_read, h->error_record, name, cap, record);
}

extern "C" int smi_bamindex_add_blocks(smi_bamindex *h, const uint64_t *coffset, const uint32_t *isize, size_t n, uint64_t end_coffset) {
    if (!h || (n && (!coffset || !isize))) {
        set_error("smi_bamindex_add_blocks: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed || h->finished) {
        set_error(h->failed ? "smi_bamindex_add_blocks: an earlier call failed" : "smi_bamindex_add_blocks: the index is finished");
        return SMI_ERR_STATE;
    }
    uint64_t at = h->next_coff;
    for (size_t k = 0; k < n; k++) {
        if (coffset[k] < at || coffset[k] >= (1ull << 48) || isize[k] > 65536u) {
            set_error("smi_bamindex_add_blocks: block " + std::to_string(k) + " is out of file order, behind 2^48 or larger than 64 KiB");
            return SMI_ERR_INVALID;
        }
        at = coffset[k] + 1;
    }
    if (end_coffset < (n ? coffset[n - 1] + 1 : h->next_coff) || end_coffset > (1ull << 48)) {
        set_error("smi_bamindex_add_blocks: end_coffset lies in front of the last block or behind 2^48");
        return SMI_ERR_INVALID;
    }
    SMI_HIP(hipSetDevice(h->ctx->device));
    for (size_t k = 0; k < n; k++) {
        if (!isize[k]) continue;  // holds no byte
        if (h->pending) {
            h->pending = false;
            if (coffset[k] != h->after_coff) {  // empty blocks stood between: the position behind the last record is in this block
                hipLaunchKernelGGL(k_bai_patch, dim3(1), dim3(1), 0, h->ctx->stream, h->d_cval, (long long)h->pending_chunk, h->meta().max_off,
                                   h->pending_ref, (unsigned long long)(coffset[k] << 16));
                SMI_HIP(hipGetLastError());
            }
        }
        h->blk_start.push_back(h->stream_total);
        h->blk_coff.push_back(coffset[k]);
        h->stream_total += isize[k];
        h->after_coff = k + 1 < n ? coffset[k + 1] : end_coffset;
        h->counts[SMI_BAI_BLOCKS]++;
    }
    h->next_coff = end_coffset;
    return SMI_OK;
}

extern "C" int smi_bamindex_add_segment(smi_bamindex *h, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n, uint64_t stream_off) {
    if (!h || n < 0 || (n && (!bam || !recs))) {
        set_error("smi_bamindex_add_segment: bad argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed || h->finished) {
        set_error(h->failed ? "smi_bamindex_add_segment: an earlier call failed" : "smi_bamindex_add_segment: the index is finished");
        return SMI_ERR_STATE;
    }
    if (!n) return SMI_OK;
    const size_t N = (size_t)n;
    // every record and its CIGAR inside the buffer, the records one behind the other: the kernels read nothing outside bam[0 .. n_bam)
    for (int32_t i = 0; i < n; i++) {
        const smi_bam_record &r = recs[i];
        if (r.rec_len < 36 || r.rec_off + r.rec_len > n_bam || r.cigar_off < r.rec_off || r.cigar_off + 4ull * r.n_cigar > r.rec_off + r.rec_len ||
            r.name_off < r.rec_off || r.name_off + r.l_read_name > r.rec_off + r.rec_len || (i && r.rec_off < recs[i - 1].rec_off + recs[i - 1].rec_len)) {
            set_error("smi_bamindex_add_segment: record index entry " + std::to_string(i) + " points outside the BAM buffer");
            return SMI_ERR_INVALID;
        }
    }
    const uint64_t first = stream_off + recs[0].rec_off, last = stream_off + recs[n - 1].rec_off + recs[n - 1].rec_len;
    if (h->blk_start.empty() || last > h->stream_total) {
        set_error("smi_bamindex_add_segment: the segment ends behind the blocks handed in (smi_bamindex_add_blocks comes first)");
        return SMI_ERR_STATE;
    }
    if (h->n_chunks + N > (uint64_t)INT32_MAX) {  // hipcub counts in int
        h->failed = true;
        set_error("BamIndex: more than 2^31 - 1 chunks and records of one segment");
        return SMI_ERR_INVALID;
    }
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    // the slice of the block table: from the block that holds the first record's first byte to the end, and the position behind
    const size_t b0 = (size_t)(std::upper_bound(h->blk_start.begin(), h->blk_start.end(), first) - h->blk_start.begin()) - 1;
    const size_t nb = h->blk_start.size() - b0 + 1;
    if (nb > (size_t)UINT32_MAX) {
        set_error("BamIndex: more than 2^32 - 1 blocks under one segment");
        return SMI_ERR_INVALID;
    }
    std::vector<uint64_t> slice(2 * nb);
    std::memcpy(slice.data(), h->blk_start.data() + b0, (nb - 1) * sizeof(uint64_t));
    std::memcpy(slice.data() + nb, h->blk_coff.data() + b0, (nb - 1) * sizeof(uint64_t));
    slice[nb - 1] = h->stream_total;
    slice[2 * nb - 1] = h->after_coff;
    std::memset(h->ms, 0, sizeof h->ms);
    if (int rc = grow(&h->d_bam, h->bam_cap, n_bam + 8)) return rc;
    if (int rc = grow(&h->d_recs, h->recs_cap, N)) return rc;
    if (int rc = grow(&h->d_rec, h->rec_cap, N)) return rc;
    if (int rc = grow(&h->d_head, h->head_cap, N)) return rc;
    if (int rc = grow(&h->d_incl, h->incl_cap, N)) return rc;
    if (int rc = grow(&h->d_blk, h->blk_cap, 2 * nb)) return rc;
    if (int rc = grow_keep(&h->d_ckey, h->ckey_cap, (size_t)h->n_chunks, (size_t)h->n_chunks + N, s)) return rc;
    if (int rc = grow_keep(&h->d_cval, h->cval_cap, (size_t)h->n_chunks, (size_t)h->n_chunks + N, s)) return rc;
    const auto scan = [&](void *p, size_t &t) { return hipcub::DeviceScan::InclusiveSum(p, t, h->d_head, h->d_incl, n, s); };
    if (int rc = reserve(h->cub, scan)) return rc;
    h->failed = true;  // until the segment is through: a call that fails half-way leaves the resident arrays in no known state
    SMI_HIP(hipMemcpyAsync(h->d_bam, bam, n_bam, hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemcpyAsync(h->d_recs, recs, N * sizeof(smi_bam_record), hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemcpyAsync(h->d_blk, slice.data(), 2 * nb * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    SMI_HIP(hipMemsetAsync(h->d_words + W_ERR, 0xff, sizeof(unsigned long long), s));
    SMI_HIP(hipMemsetAsync(h->d_words + W_NO_COOR, 0, sizeof(unsigned long long), s));
    // stage 1
    if (int rc = h->ev.begin(s)) return rc;
    {
        RecArgs a = {h->d_bam, h->d_recs, (uint32_t)n, h->n_ref, stream_off, h->d_blk, h->d_blk + nb, (uint32_t)nb, h->d_win_cap, h->d_rec, h->d_words};
        hipLaunchKernelGGL(k_bai_rec, dim3(grid(N, kBaiRecs)), dim3(kBaiBlock), 0, s, a);
        SMI_HIP(hipGetLastError());
    }
    if (int rc = h->ev.end(s, &h->ms[0])) return rc;
    // stage 2
    if (int rc = h->ev.begin(s)) return rc;
    hipLaunchKernelGGL(k_bai_order, dim3(grid(N)), dim3(kBaiBlock), 0, s, h->d_rec, (uint32_t)n, (const Carry *)h->d_carry, h->d_head, h->meta(), h->d_words);
    SMI_HIP(hipGetLastError());
    if (int rc = run_reserved(h->cub, scan)) return rc;
    if (int rc = h->ev.end(s, &h->ms[1])) return rc;
    unsigned long long words[W_COUNT] = {};
    uint32_t heads = 0;
    SMI_HIP(hipMemcpyAsync(words, h->d_words, sizeof words, hipMemcpyDeviceToHost, s));
    SMI_HIP(hipMemcpyAsync(&heads, h->d_incl + (N - 1), sizeof heads, hipMemcpyDeviceToHost, s));
    SMI_HIP(hipStreamSynchronize(s));
    if (words[W_ERR] != kNoRecord) {
        const smi_bam_record &r = recs[words[W_ERR]];
        BaiRec c;
        SMI_HIP(hipMemcpy(&c, h->d_rec + words[W_ERR], sizeof c, hipMemcpyDeviceToHost));
        h->error_read.assign((const char *)bam + r.name_off, r.l_read_name ? r.l_read_name - 1u : 0u);
        h->error_record = h->counts[SMI_BAI_RECORDS] + (int64_t)words[W_ERR];
        set_error("read " + h->error_read + " (record " + std::to_string(h->error_record) + "): " + kStopText[std::min<uint32_t>(c.flags >> BAI_KIND_SHIFT, 5u)]);
        return 2;
    }
    // stages 3 and 4
    if (int rc = h->ev.begin(s)) return rc;
    hipLaunchKernelGGL(k_bai_chunk, dim3(grid(N)), dim3(kBaiBlock), 0, s, (const BaiRec *)h->d_rec, (uint32_t)n, (const uint32_t *)h->d_head,
                       (const uint32_t *)h->d_incl, h->n_chunks, (uint64_t)std::min(h->ckey_cap, h->cval_cap), h->d_ckey, h->d_cval, h->d_carry);
    SMI_HIP(hipGetLastError());
    if (int rc = h->ev.end(s, &h->ms[2])) return rc;
    if (int rc = h->ev.begin(s)) return rc;
    hipLaunchKernelGGL(k_bai_lin, dim3(grid(N, kBaiRecs)), dim3(kBaiBlock), 0, s, (const BaiRec *)h->d_rec, (uint32_t)n, (const uint64_t *)h->d_win_off, h->d_lin);
    SMI_HIP(hipGetLastError());
    if (int rc = h->ev.end(s, &h->ms[3])) return rc;
    h->n_chunks += heads;
    h->pending = last == h->stream_total;
    h->pending_ref = recs[n - 1].ref_id >= 0 ? recs[n - 1].ref_id : -1;
    h->pending_chunk = h->pending_ref >= 0 ? (int64_t)h->n_chunks - 1 : -1;
    h->counts[SMI_BAI_RECORDS] += n;
    h->counts[SMI_BAI_NO_COOR] += (int64_t)words[W_NO_COOR];
    h->counts[SMI_BAI_CHUNKS] = (int64_t)h->n_chunks;
    h->counts[SMI_BAI_SEGMENTS]++;
    h->failed = false;
    return SMI_OK;
}

namespace {

void put32(std::string &s, uint32_t v) { s.append((const char *)&v, 4); }
void put64(std::string &s, uint64_t v) { s.append((const char *)&v, 8); }

// the sorted arrays -> the file's layout
int bai_finish(smi_bamindex *h) {
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    const size_t n = (size_t)std::max(h->n_ref, 1), nc = (size_t)h->n_chunks, n_win = (size_t)h->win_off[n];
    std::memset(h->ms, 0, sizeof h->ms);
    DevBuf<unsigned long long> skey("BamIndex"), ukey("BamIndex");
    DevBuf<Voff> sval("BamIndex");
    DevBuf<uint32_t> ucount("BamIndex"), n_runs("BamIndex");
    if (int rc = skey.alloc(nc)) return rc;
    if (int rc = ukey.alloc(nc)) return rc;
    if (int rc = sval.alloc(nc)) return rc;
    if (int rc = ucount.alloc(nc)) return rc;
    if (int rc = n_runs.alloc(1)) return rc;
    SMI_HIP(hipMemsetAsync(n_runs.p, 0, sizeof(uint32_t), s));
    if (int rc = h->ev.begin(s)) return rc;
    const Meta m = h->meta();
    if (nc) {
        int ref_bits = 1;
        while (ref_bits < 31 && (1ll << ref_bits) < h->n_ref) ref_bits++;
        const auto sort = [&](void *p, size_t &t) { return hipcub::DeviceRadixSort::SortPairs(p, t, h->d_ckey, skey.p, h->d_cval, sval.p, (int)nc, 0, 32 + ref_bits, s); };
        const auto bins = [&](void *p, size_t &t) { return hipcub::DeviceRunLengthEncode::Encode(p, t, skey.p, ukey.p, ucount.p, n_runs.p, (int)nc, s); };
        if (int rc = reserve(h->cub, sort, bins)) return rc;
        if (int rc = run_reserved(h->cub, sort)) return rc;
        if (int rc = run_reserved(h->cub, bins)) return rc;
        hipLaunchKernelGGL(k_bai_bins, dim3(grid(nc)), dim3(kBaiBlock), 0, s, (const unsigned long long *)ukey.p, (const uint32_t *)n_runs.p, m.n_bin);
        SMI_HIP(hipGetLastError());
    }
    if (h->n_ref) {
        hipLaunchKernelGGL(k_bai_fill, dim3((unsigned)h->n_ref), dim3(kBaiBlock), 0, s, h->d_lin, (const uint64_t *)h->d_win_off, (const uint32_t *)m.max_end);
        SMI_HIP(hipGetLastError());
    }
    if (int rc = h->ev.end(s, &h->ms[4])) return rc;
    uint32_t runs = 0;
    SMI_HIP(hipMemcpy(&runs, n_runs.p, sizeof runs, hipMemcpyDeviceToHost));
    std::vector<unsigned long long> key(runs), meta64(4 * n), lin(n_win);
    std::vector<uint32_t> count(runs), meta32(2 * n);
    std::vector<Voff> val(nc);
    if (runs) SMI_HIP(hipMemcpyAsync(key.data(), ukey.p, runs * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (runs) SMI_HIP(hipMemcpyAsync(count.data(), ucount.p, runs * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (nc) SMI_HIP(hipMemcpyAsync(val.data(), sval.p, nc * sizeof(Voff), hipMemcpyDeviceToHost, s));
    if (n_win) SMI_HIP(hipMemcpyAsync(lin.data(), h->d_lin, n_win * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    SMI_HIP(hipMemcpyAsync(meta64.data(), h->d_meta64, 4 * n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    SMI_HIP(hipMemcpyAsync(meta32.data(), h->d_meta32, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    SMI_HIP(hipStreamSynchronize(s));
    std::string &o = h->bai;
    o.assign("BAI\1", 4);
    put32(o, (uint32_t)h->n_ref);
    size_t run = 0, chunk = 0;
    int64_t with_records = 0, windows = 0;
    for (int32_t r = 0; r < h->n_ref; r++) {
        const uint64_t records = meta64[2 * n + r] + meta64[3 * n + r];
        const uint32_t n_bin = meta32[n + r];
        put32(o, n_bin + (records ? 1u : 0u));
        for (uint32_t b = 0; b < n_bin; b++, run++) {
            if (run >= runs || (int32_t)(key[run] >> 32) != r) {  // (cannot happen: n_bin counts these runs)
                set_error("BamIndex: the sorted chunks do not match the bins per reference");
                return SMI_ERR_STATE;
            }
            put32(o, (uint32_t)key[run]);
            put32(o, count[run]);
            for (uint32_t c = 0; c < count[run]; c++, chunk++) {
                put64(o, val[chunk].beg);
                put64(o, val[chunk].end);
            }
        }
        uint32_t n_intv = 0;
        if (records) {
            with_records++;
            put32(o, kMetaBin);
            put32(o, 2);
            put64(o, meta64[r]);
            put64(o, meta64[n + r]);
            put64(o, meta64[2 * n + r]);
            put64(o, meta64[3 * n + r]);
            n_intv = ((meta32[r] - 1) >> 14) + 1;
        }
        put32(o, n_intv);
        o.append((const char *)(lin.data() + h->win_off[r]), 8ull * n_intv);
        windows += n_intv;
    }
    if (run != runs || chunk != nc) {
        set_error("BamIndex: the sorted chunks do not match the bins per reference");
        return SMI_ERR_STATE;
    }
    put64(o, (uint64_t)h->counts[SMI_BAI_NO_COOR]);
    h->counts[SMI_BAI_REFS_WITH_RECORDS] = with_records;
    h->counts[SMI_BAI_BINS] = (int64_t)runs;
    h->counts[SMI_BAI_WINDOWS] = windows;
    return SMI_OK;
}

}  // namespace

extern "C" int smi_bamindex_finish(smi_bamindex *h, uint8_t *out, size_t cap, size_t *n_out) {
    if (!h || !n_out) {
        set_error("smi_bamindex_finish: null argument");
        return SMI_ERR_INVALID;
    }
    *n_out = 0;
    if (h->failed) {
        set_error("smi_bamindex_finish: an earlier call failed");
        return SMI_ERR_STATE;
    }
    if (!h->finished) {
        if (int rc = bai_finish(h)) {
            h->failed = true;
            return rc;
        }
        h->finished = true;
    }
    return handle::get_text(h->bai, out, cap, n_out);
}
