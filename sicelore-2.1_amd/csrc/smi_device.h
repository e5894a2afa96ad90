// smi_device.h -- the device side the file programs share (smi_handle.h is its host twin): hipcub's temporary storage and the two-call
// protocol, the probe of the byte-key grouping tables, and the wave and byte helpers.  (The attribute-size rule, lr::aux_size, is in
// smi_longread.h, which a plain C++ compiler builds too.)
#pragma once
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "smi_internal.h"

namespace smi {

// ---- hipcub ---------------------------------------------------------------------------------------------------------------------------
// A hipcub call is written once per site, as a callable  hipError_t f(void *tmp, size_t &tmp_bytes)  that passes both on:
//   auto scan = [&](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, in, out, n, s); };
// reserve() asks each callable for its size (tmp == nullptr launches nothing) and grows the scratch to the largest; run() does the same
// for one callable and then calls it.  A site inside a timed bracket reserves in front of the bracket and calls run_reserved() inside it,
// which asks and allocates nothing (hipcub refuses a scratch that is too small: a forgotten reserve() is an error, not a fault).

// grow-only device scratch; who: the program named when the allocation fails.  It grows with a quarter to spare: hipcub's sizes step up
// with the item count, and a handle that keeps its scratch across segments must not allocate for every segment a little larger than the last
struct Scratch {
    DevBuf<uint8_t> b;
    size_t cap = 0;
    explicit Scratch(const char *who) : b(who) {}
    int need(size_t n) {
        if (n <= cap && b.p) return SMI_OK;
        cap = 0;
        const size_t grown = std::max<size_t>(n + n / 4, 1024);
        if (int rc = b.alloc(grown)) return rc;
        cap = grown;
        return SMI_OK;
    }
};

template <class... F>
int reserve(Scratch &t, const F &...f) {
    size_t most = 0;
    hipError_t e = hipSuccess;
    auto ask = [&](const auto &g) {
        size_t n = 0;
        const hipError_t r = g(nullptr, n);
        most = std::max(most, n);
        if (e == hipSuccess) e = r;
    };
    (ask(f), ...);
    SMI_HIP(e);
    return t.need(most);
}

template <class F>
int run_reserved(Scratch &t, const F &f) {
    size_t n = t.cap;
    SMI_HIP(f(t.b.p, n));
    return SMI_OK;
}
template <class F>
int run(Scratch &t, const F &f) {
    if (int rc = reserve(t, f)) return rc;
    return run_reserved(t, f);
}

// Radix sort of n 64-bit codes on bits [0, end_bit), then run-length encoding: `unique` = the distinct codes in order, cnt = how often
// each occurs, *n_run = how many there are (all device memory; `sorted` is the scratch between the two).
template <class Cnt, class Runs>
struct SortRle {
    const uint64_t *in;
    uint64_t *sorted, *unique;
    Cnt *cnt;
    Runs *n_run;
    int n, end_bit;
    hipStream_t s;
    auto sort() const {
        return [*this](void *p, size_t &t) { return hipcub::DeviceRadixSort::SortKeys(p, t, in, sorted, n, 0, end_bit, s); };
    }
    auto encode() const {
        return [*this](void *p, size_t &t) { return hipcub::DeviceRunLengthEncode::Encode(p, t, sorted, unique, cnt, n_run, n, s); };
    }
    int reserve(Scratch &t) const { return smi::reserve(t, sort(), encode()); }
    int run_reserved(Scratch &t) const {
        if (int rc = smi::run_reserved(t, sort())) return rc;
        return smi::run_reserved(t, encode());
    }
    int run(Scratch &t) const {
        if (int rc = reserve(t)) return rc;
        return run_reserved(t);
    }
};
template <class Cnt, class Runs>
SortRle<Cnt, Runs> sort_rle(hipStream_t s, const uint64_t *in, uint64_t *sorted, uint64_t *unique, Cnt *cnt, Runs *n_run, int n, int end_bit) {
    return {in, sorted, unique, cnt, n_run, n, end_bit, s};
}

// ---- byte keys ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool same_bytes(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint32_t n) {
    for (uint32_t k = 0; k < n; k++)
        if (a[k] != b[k]) return false;
    return true;
}

// 64-bit FNV-1a: fnv1a_add takes one more byte into h (host too: a table built on the host is probed with the same function)
constexpr uint64_t kFnvBasis = 14695981039346656037ull;
__host__ __device__ __forceinline__ uint64_t fnv1a_add(uint64_t h, uint8_t c) { return (h ^ c) * 1099511628211ull; }
__device__ __forceinline__ uint64_t fnv1a(const uint8_t *__restrict__ p, uint32_t n) {
    uint64_t h = kFnvBasis;
    for (uint32_t k = 0; k < n; k++) h = fnv1a_add(h, p[k]);
    return h;
}

constexpr uint32_t kEmpty = 0xffffffffu;  // a free slot of a grouping table

struct Bytes {
    const uint8_t *p;
    uint32_t n;
};
struct Probed {
    uint32_t entry;  // the entry that holds the key, kEmpty: none (LOOKUP), or no room in one turn round the table
    uint32_t steps, wraps;
};

// One key's walk through an open-addressing table (mask + 1 slots of entry numbers) from `slot` on, by linear probing.  An entry e stands
// for the bytes key_of(e) (a Bytes); the walk ends at the entry whose bytes equal `mine`, or, INSERT, at the free slot it claims for `me`
// by CAS.  Which of several equal keys claims the slot is a race; the callers' results do not depend on it.
template <bool INSERT, class KeyOf>
__device__ __forceinline__ Probed probe(uint32_t *__restrict__ tab, uint32_t mask, uint32_t slot, uint32_t me, Bytes mine, const KeyOf key_of) {
    Probed o = {kEmpty, 0, 0};
    while (o.steps <= mask) {  // at most one turn round the table
        uint32_t cur = __hip_atomic_load(&tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmpty) {
            if (!INSERT) break;
            cur = atomicCAS(&tab[slot], kEmpty, me);
            if (cur == kEmpty) {
                o.entry = me;
                break;
            }
        }
        const Bytes theirs = key_of(cur);
        if (theirs.n == mine.n && same_bytes(mine.p, theirs.p, mine.n)) {
            o.entry = cur;
            break;
        }
        slot = (slot + 1) & mask;
        o.steps++;
        o.wraps += slot == 0;
    }
    return o;
}

// ---- wave and byte helpers ------------------------------------------------------------------------------------------------------------
// all lanes: dst[0 .. n) = src[0 .. n); the destination's dwords are stored whole
__device__ __forceinline__ void wave_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t n, int lane) {
    const uint64_t to_dword = (4 - ((uintptr_t)dst & 3)) & 3, head = n < to_dword ? n : to_dword;
    if ((uint64_t)lane < head) dst[lane] = src[lane];
    const uint64_t words = (n - head) >> 2;
    for (uint64_t k = lane; k < words; k += 64) {
        uint32_t w;
        __builtin_memcpy(&w, src + head + 4 * k, 4);
        *reinterpret_cast<uint32_t *>(dst + head + 4 * k) = w;
    }
    const uint64_t done = head + 4 * words;
    if (done + lane < n) dst[done + lane] = src[done + lane];
}

// The copy K-SORT-GATHER, K-MERGE-GATHER (smi_bamsort.hip) and K-VIEW-GATHER (smi_bamview.hip) share: the L bytes at s to dst + d0, where
// dst is aligned to 256 bytes, by the kCopyLanes lanes of a group (sub: the lane's number in it).  The bytes in front of the first
// W-aligned destination address and those behind the last one go one byte per lane (fewer than W <= kCopyLanes of either), the body in
// W-byte words: a store aligned to W, a load of any alignment.  Every load and store lies inside the record.
constexpr int kCopyLanes = 16;
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
template <int W>
__device__ __forceinline__ void copy_record(const uint8_t *__restrict__ s, uint32_t L, uint64_t d0, uint8_t *__restrict__ dst, uint32_t sub) {
    using T = typename Word<W>::type;
    static_assert(W <= kCopyLanes, "head and tail go one byte per lane");
    uint8_t *__restrict__ d = dst + d0;
    const uint32_t want = (uint32_t)(-(int64_t)d0) & (W - 1), head = want < L ? want : L;
    const uint32_t words = (L - head) / W, tail = (L - head) % W, tail_at = head + words * W;
    if (sub < head) d[sub] = s[sub];
    for (uint32_t w = sub; w < words; w += kCopyLanes) {
        T v;
        __builtin_memcpy(&v, s + head + (size_t)w * W, W);
        *reinterpret_cast<T *>(__builtin_assume_aligned(d + head + (size_t)w * W, W)) = v;
    }
    if (sub < tail) d[tail_at + sub] = s[tail_at + sub];
}

// inclusive prefix sum across the wave
template <class T>
__device__ __forceinline__ T wave_incl_sum(T v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        T y;
        if constexpr (sizeof(T) == 8) y = (T)__shfl_up((long long)v, o);
        else y = __shfl_up(v, o);
        if (lane >= o) v += y;
    }
    return v;
}

// decimal digits of v
__device__ __forceinline__ int digits(uint32_t v) {
    int n = 1;
    while (v >= 10) {
        v /= 10;
        n++;
    }
    return n;
}

// little-endian 32-bit words at any alignment
__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
__device__ __forceinline__ void st_u32(uint8_t *p, uint32_t v) {
    for (int k = 0; k < 4; k++) p[k] = (uint8_t)(v >> (8 * k));
}

// two junctions within d of each other at both ends; isIn(j, lst, DELTA) of the reference's UCSCRefFlatParser
__device__ __forceinline__ bool near(int2 a, int2 b, int d) { return abs(a.x - b.x) <= d && abs(a.y - b.y) <= d; }
__device__ __forceinline__ bool is_in(int2 j, const int2 *__restrict__ lst, int n, int d) {
    for (int i = 0; i < n; i++)
        if (near(lst[i], j, d)) return true;
    return false;
}

}  // namespace smi
