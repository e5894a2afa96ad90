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
