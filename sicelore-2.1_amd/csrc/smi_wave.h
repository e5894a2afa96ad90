// smi_wave.h -- numbering and queueing of work items inside ONE wavefront: shared by K-SCAN (smi_scan.hip: alignment candidates) and K-BC1
// (smi_bc.hip: bucket look-ups).  Lanes that own a varying number of items number them through a prefix sum and push them into 64 slots per
// round, so that the work behind runs with full waves whatever the per-owner counts are.
#pragma once
#include "smi_internal.h"

// variant switch for counter runs and cross-checks (make VARIANT=... EXTRA=-DSMI_SCAN_SHFL_SCAN=1), never set in the shipped library:
// the wave prefix sum through six __shfl_up steps (ds_bpermute) instead of DPP
#ifndef SMI_SCAN_SHFL_SCAN
#define SMI_SCAN_SHFL_SCAN 0
#endif

namespace smi {

// ---- work units taken by the wave (K-SCAN: tiles of 64 read ends) ---------------------------------------------------------------------------------
// The units 0 .. n - 1 of a launch are cut into kClaimShards consecutive ranges with a head counter each (heads[s * kClaimStride], set to 0 on the
// launch's stream: claim_counters() in smi_ctx.hip).  A wave takes units from the range of its block's shard with one returning atomicAdd by lane 0
// and, when that range has run out, from the next range that has units left (one load of all heads by the first lanes finds it).  One head for the
// whole launch was measured first: a device-scope atomic on ONE word is served every ~ 12 ns, the device finishes a tile every 6 ns, and the
// kernel ran at the atomic's rate (K-SCAN 1.90 -> 3.79 ms; K-BC1, whose claim loop was not kept, 0.59 -> 1.86 ms: NOTES R6.36).
constexpr int kClaimShards = 16;
struct WaveClaim {
    uint32_t *heads;
    uint32_t n, per;  // units of the launch, units per shard (the last shards may hold fewer, or none)
    uint32_t shard;   // the range this wave takes from now (wave-uniform)
    __device__ __forceinline__ uint32_t len(uint32_t s) const { return s * per >= n ? 0u : min(per, n - s * per); }
    // lane 0 asks for the next unit of the wave's shard; the answer is read by take()
    __device__ __forceinline__ uint32_t ask(int lane) const {
        uint32_t v = 0;
        if (lane == 0) v = atomicAdd(heads + shard * kClaimStride, 1u);
        return v;
    }
    // the unit an answer stands for, or n when no range has a unit left (every lane of the wave calls this; the result is wave-uniform)
    __device__ __forceinline__ uint32_t take(uint32_t answer, int lane) {
        uint32_t rel = (uint32_t)__builtin_amdgcn_readfirstlane((int)answer);
        while (rel >= len(shard)) {
            uint32_t head = 0xFFFFFFFFu;
            if (lane < kClaimShards) head = __hip_atomic_load(heads + lane * kClaimStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t open = __ballot(lane < kClaimShards && head < len((uint32_t)lane));
            if (!open) return n;
            // the first open range behind this one, cyclically
            const uint64_t behind = open & ~((2ull << shard) - 1ull);
            shard = (uint32_t)__builtin_ctzll(behind ? behind : open);
            rel = (uint32_t)__builtin_amdgcn_readfirstlane((int)ask(lane));
        }
        return shard * per + rel;
    }
};
__device__ __forceinline__ WaveClaim wave_claim_init(uint32_t *heads, uint32_t n_units) {
    WaveClaim c;
    c.heads = heads, c.n = n_units, c.per = (n_units + kClaimShards - 1) / kClaimShards;
    c.shard = blockIdx.x % kClaimShards;
    return c;
}

// wave-wide exclusive prefix sum of one int per lane; returns the wave total (wave-uniform) through `total`.  Called with all 64 lanes active.
__device__ __forceinline__ int wave_exscan(int v, int lane, int &total) {
    int inc = v;
#if SMI_SCAN_SHFL_SCAN
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
    }
    total = __builtin_amdgcn_readfirstlane(__shfl(inc, 63));
#else
    // DPP: a Hillis-Steele sum inside each row of 16 lanes (row_shr:1/2/4/8, lanes without a source add 0), then lane 15 of a row into the
    // row behind it (row_bcast:15 on rows 1 and 3) and lane 31 into rows 2 and 3 (row_bcast:31): eight VALU operations, no LDS crossbar
    (void)lane;
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xf, 0xf, true);   // row_shr:1
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xf, 0xf, true);   // row_shr:2
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xf, 0xf, true);   // row_shr:4
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xf, 0xf, true);   // row_shr:8
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x142, 0xa, 0xf, false);  // row_bcast:15 row_mask:0xa
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x143, 0xc, 0xf, false);  // row_bcast:31 row_mask:0xc
    total = __builtin_amdgcn_readlane(inc, 63);
#endif
    return inc - v;
}

// Owner push of the candidate queue.  The candidates of a wave are numbered off + k for the k-th set bit of the owner's masks (chunk order, then
// bit order), and round `base` aligns the numbers [base, base + 64) on lanes 0 .. 63.  An owner whose numbers [off, off + n) meet the round walks
// its set bits and writes `lane | value << 8` into the slot of each of those candidates (slots = the wave's 64 words of `coff`); the candidate
// lane reads one word.  `mask_of(ch)` hands over the owner's mask of chunk ch, `value(ch, bit)` what the candidate needs (<= 255: the shift by 8
// leaves the lane bits alone).  -> nothing; the caller puts wave_sync() between this and the candidates' read.
template <int CH, typename M, typename V>
__device__ __forceinline__ void queue_push(uint32_t *slots, int lane, int off, int n, int base, M mask_of, V value) {
    const int f0 = max(off, base), f1 = min(off + n, base + 64);
    if (f0 < f1) {
        int idx = off;
#pragma unroll
        for (int ch = 0; ch < CH; ch++) {
            uint64_t m = mask_of(ch);
            while (m != 0ull && idx < f1) {
                const int bit = __builtin_ctzll(m);
                m &= m - 1;
                if (idx >= f0) slots[idx - base] = (uint32_t)lane | ((uint32_t)value(ch, bit) << 8);
                idx++;
            }
        }
    }
}

}  // namespace smi
