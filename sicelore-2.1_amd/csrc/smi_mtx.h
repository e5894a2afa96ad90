// smi_mtx.h -- K-MTX, the dense count matrices of Matrix.writeIsoformMatrix / writeGeneMatrix / writeJunctionMatrix (Matrix.java L158-290),
// shared by IsoformMatrix (smi_isoform.hip) and SNPMatrix (smi_snp.hip): 64-bit (row << 32 | cell) codes, one per counted UMI; hipcub radix
// sort + run-length encoding give the counts per (row, cell); the dense rows are rendered in row blocks under a device-memory budget, one
// wavefront per row: a length pass, a scan, the write.  (DevBuf and Events are in smi_internal.h, the hipcub scratch, sort_rle and the wave
// helpers in smi_device.h.)
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "smi_device.h"

namespace smi {
namespace mtx {

constexpr int kRenderWaves = 4;  // waves per block of the renderer

// dense[(row - r0) * nc + cell] = count, for the runs of rows r0 ..
static __global__ void k_mtx_scatter(const uint64_t *__restrict__ code, const uint32_t *__restrict__ cnt, int64_t k0, int64_t k1, int32_t r0, int32_t nc,
                              uint32_t *__restrict__ dense) {
    const int64_t k = k0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k >= k1) return;
    const uint64_t c = code[k];
    dense[(int64_t)((int32_t)(c >> 32) - r0) * nc + (uint32_t)c] = cnt[k];
}

// LEN: bytes of row r0 + i (label, "\t" + count per cell, "\n") into len[i]; WRITE: the row at off[i]
template <bool WRITE>
__global__ __launch_bounds__(64 * kRenderWaves) void k_mtx_render(const uint32_t *__restrict__ dense, int32_t n_rows, int32_t nc, int32_t r0,
                                                                   const uint8_t *__restrict__ labels, const uint64_t *__restrict__ lab_off,
                                                                   uint64_t *__restrict__ len, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kRenderWaves + (threadIdx.x >> 6);
    if (i >= n_rows) return;
    const uint32_t *row = dense + (int64_t)i * nc;
    const uint64_t l0 = lab_off[r0 + i], ln = lab_off[r0 + i + 1] - l0;
    if (!WRITE) {
        uint64_t n = 0;
        for (int c = lane; c < nc; c += 64) n += 1 + digits(row[c]);
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
        if (lane == 0) len[i] = n + ln + 1;
        return;
    }
    uint8_t *dst = out + len[i];  // (the exclusive scan of the lengths)
    for (uint64_t k = lane; k < ln; k += 64) dst[k] = labels[l0 + k];
    uint64_t pos = ln;
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int c = c0 + lane;
        const uint32_t v = c < nc ? row[c] : 0;
        const int w = c < nc ? 1 + digits(v) : 0;
        const int incl = wave_incl_sum(w, lane);
        if (c < nc) {
            uint8_t *p = dst + pos + (incl - w);
            p[0] = '\t';
            uint32_t x = v;
            for (int k = w - 1; k >= 1; k--) {
                p[k] = (uint8_t)('0' + x % 10);
                x /= 10;
            }
        }
        pos += __shfl(incl, 63);
    }
    if (lane == 0) dst[pos] = '\n';
}

// K-MTX for one matrix: codes (row << 32 | cell), one per counted UMI -> counts per (row, cell) (sorted codes, device) and the dense rows
// of `labels` x nc cells appended to dst, rendered in blocks of at most budget_bytes (0: 1 GiB) of device memory; row_total: the sum of
// each row; *blocks is raised by the row blocks rendered.  who: the program named in an error.
inline int matrix(hipStream_t s, const char *who, int32_t nc, int64_t budget_bytes, std::vector<uint64_t> &codes, const std::vector<std::string> &labels,
                  std::string &dst, std::vector<int64_t> &row_total, float *ms_sort, float *ms_render, int64_t *blocks) {
    const int64_t nrows = (int64_t)labels.size();
    row_total.assign(nrows, 0);
    const size_t n = codes.size();
    std::vector<uint64_t> ucode;
    std::vector<uint32_t> ucnt;
    Events ev;
    if (n > (size_t)INT32_MAX) {
        set_error(std::string(who) + ": " + std::to_string(n) + " matrix entries in one matrix; at most 2^31 - 1 are counted in one sort");
        return SMI_ERR_INVALID;
    }
    int end_bit = 32;  // cells < 2^31 in the low word; the row in as many bits above as the rows need
    while (end_bit < 64 && ((uint64_t)1 << (end_bit - 32)) < (uint64_t)nrows) end_bit++;
    if (n) {
        DevBuf<uint64_t> d_in{who}, d_sorted{who}, d_unique{who};
        DevBuf<uint32_t> d_cnt{who};
        DevBuf<int64_t> d_nrun{who};
        Scratch tmp{who};
        if (int rc = d_in.put(codes, s)) return rc;
        if (int rc = d_sorted.alloc(n)) return rc;
        if (int rc = d_unique.alloc(n)) return rc;
        if (int rc = d_cnt.alloc(n)) return rc;
        if (int rc = d_nrun.alloc(1)) return rc;
        const auto count = sort_rle(s, d_in.p, d_sorted.p, d_unique.p, d_cnt.p, d_nrun.p, (int)n, end_bit);
        if (int rc = count.reserve(tmp)) return rc;
        if (int rc = ev.begin(s)) return rc;
        if (int rc = count.run_reserved(tmp)) return rc;
        if (int rc = ev.end(s, ms_sort)) return rc;
        int64_t nrun = 0;
        SMI_HIP(hipMemcpy(&nrun, d_nrun.p, sizeof(nrun), hipMemcpyDeviceToHost));
        ucode.resize(nrun);
        ucnt.resize(nrun);
        SMI_HIP(hipMemcpy(ucode.data(), d_unique.p, nrun * sizeof(uint64_t), hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(ucnt.data(), d_cnt.p, nrun * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    for (size_t k = 0; k < ucode.size(); k++) row_total[ucode[k] >> 32] += ucnt[k];
    if (nrows == 0) return SMI_OK;
    // labels back to back; the largest count gives the widest field
    std::vector<uint8_t> lab;
    std::vector<uint64_t> lab_off{0};
    for (auto &l : labels) {
        lab.insert(lab.end(), l.begin(), l.end());
        lab_off.push_back(lab.size());
    }
    uint32_t maxc = 0;
    for (uint32_t x : ucnt) maxc = std::max(maxc, x);
    const int wd = 1 + (int)std::to_string(maxc).size();
    const int64_t budget = budget_bytes > 0 ? budget_bytes : (int64_t)1 << 30;
    DevBuf<uint8_t> d_lab{who};
    DevBuf<uint64_t> d_lab_off{who}, d_ucode{who};
    DevBuf<uint32_t> d_ucnt{who};
    if (int rc = d_lab.put(lab, s)) return rc;
    if (int rc = d_lab_off.put(lab_off, s)) return rc;
    if (int rc = d_ucode.put(ucode, s)) return rc;
    if (int rc = d_ucnt.put(ucnt, s)) return rc;
    Scratch tmp{who};  // the blocks' scans
    int64_t r0 = 0;
    size_t k0 = 0;
    while (r0 < nrows) {
        // rows of this block: dense counts + the widest rendering of each row within the budget (at least one row)
        int64_t r1 = r0, bytes = 0;
        while (r1 < nrows) {
            const int64_t rb = (int64_t)nc * 4 + (int64_t)(lab_off[r1 + 1] - lab_off[r1]) + (int64_t)nc * wd + 1 + 8;
            if (r1 > r0 && bytes + rb > budget) break;
            bytes += rb;
            r1++;
        }
        const int32_t nb = (int32_t)(r1 - r0);
        size_t k1 = k0;
        while (k1 < ucode.size() && (int64_t)(ucode[k1] >> 32) < r1) k1++;
        DevBuf<uint32_t> d_dense{who};
        DevBuf<uint64_t> d_len{who}, d_off{who};
        DevBuf<uint8_t> d_out{who};
        if (int rc = d_dense.alloc((size_t)nb * std::max(nc, 1))) return rc;
        if (int rc = d_len.alloc(nb + 1)) return rc;
        if (int rc = d_off.alloc(nb + 1)) return rc;
        const auto scan = [&](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, d_len.p, d_off.p, nb + 1, s); };
        if (int rc = reserve(tmp, scan)) return rc;
        if (int rc = ev.begin(s)) return rc;
        SMI_HIP(hipMemsetAsync(d_dense.p, 0, (size_t)nb * std::max(nc, 1) * 4, s));
        SMI_HIP(hipMemsetAsync(d_len.p, 0, (nb + 1) * sizeof(uint64_t), s));
        if (k1 > k0)
            hipLaunchKernelGGL(k_mtx_scatter, dim3((unsigned)((k1 - k0 + 255) / 256)), dim3(256), 0, s, d_ucode.p, d_ucnt.p, (int64_t)k0, (int64_t)k1,
                               (int32_t)r0, nc, d_dense.p);
        const unsigned gb = (unsigned)((nb + kRenderWaves - 1) / kRenderWaves);
        hipLaunchKernelGGL(k_mtx_render<false>, dim3(gb), dim3(64 * kRenderWaves), 0, s, d_dense.p, nb, nc, (int32_t)r0, d_lab.p, d_lab_off.p,
                           d_len.p, (uint8_t *)nullptr);
        SMI_HIP(hipGetLastError());
        if (int rc = run_reserved(tmp, scan)) return rc;
        uint64_t total = 0;
        SMI_HIP(hipMemcpyAsync(&total, d_off.p + nb, sizeof(total), hipMemcpyDeviceToHost, s));
        SMI_HIP(hipStreamSynchronize(s));
        if (int rc = d_out.alloc(total)) return rc;
        hipLaunchKernelGGL(k_mtx_render<true>, dim3(gb), dim3(64 * kRenderWaves), 0, s, d_dense.p, nb, nc, (int32_t)r0, d_lab.p, d_lab_off.p,
                           d_off.p, d_out.p);
        SMI_HIP(hipGetLastError());
        const size_t at = dst.size();
        dst.resize(at + total);
        SMI_HIP(hipMemcpyAsync(&dst[at], d_out.p, total, hipMemcpyDeviceToHost, s));
        if (int rc = ev.end(s, ms_render)) return rc;
        if (blocks) (*blocks)++;
        r0 = r1;
        k0 = k1;
    }
    return SMI_OK;
}

}  // namespace mtx
}  // namespace smi
