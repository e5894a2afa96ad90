// smi_dedup.hip -- `DeduplicateMolecule` (org/ipmc/sicelore/programs/DeduplicateMolecule.java:L41-302, utils/Molecule.java:L40-60): one
// record per molecule out of the concatenated consensus FASTQ / FASTA files.  The rules are DESIGN.md section 8f's; tests/dedupmodel.py
// implements the same ones.  A streaming filter in two passes over the text, which comes in segments of any size:
//
// pass 1 (smi_dedup_add_segment), per segment:
//   line table: K-FQ's sweep through launch_fastq_sweep / launch_fastq_line_starts (smi_fastq.hip), nothing of K-FQ's record rules.
//   K-DD-STATE: the reference's reader (L186-190, L114-116) is a state machine over the lines -- FASTQ: state 0 outside a record, an '@'
//     line there starts one and the three lines behind it are consumed whatever they begin with (states 1, 2, 3); FASTA: '>' and one
//     line.  Every line is one of two transition functions, packed 2 bits per state in a byte; an inclusive hipcub scan under function
//     composition gives every line the state in front of it.  A record starts where that state is 0 and the line starts with the marker.
//   K-DD-PARSE: one thread per record start, two launches (count, hipcub exclusive scans, write): the `null` test (L192), the name
//     (L202-206: every marker removed, then backslash + '|' -> '-', then Java's split on '-'), rn = Integer(ids[2]), 64-bit FNV-1a of
//     ids[0] + ids[1]; the key bytes are appended to a device pool and the record's fields to a device table, both kept across segments.
//     The smallest offending line number is kept by an atomic minimum.
// smi_dedup_select, once the record count is known:
//   K-DD-INSERT: open addressing over a table of a power of two >= 2 x records, walked by probe() of smi_device.h; a record claims an
//     empty slot by CAS of its index, or joins the slot's representative when length and bytes of the two keys are equal (compared in
//     the pool), or probes on.  Which
//     record of a group becomes its representative is a race; the group's accumulators are indexed by it and nothing else depends on it.
//   K-DD-PICK: FASTQ with SELECT (L208-217): 64-bit atomicMax of rn << 32 | sequence length per group, then atomicMin of the index among
//     the records that equal it.  FASTA (L128-136; the four-argument Molecule constructor leaves consensusLength 0, so an equal rn
//     replaces whenever the new sequence is not empty): atomicMax of rn, then the smallest index and the largest index with a non-empty
//     sequence among the records that equal it.  SELECT=false (L285): atomicMin of the index.
//   layout: the output size of every winner, 0 for the rest, one hipcub exclusive scan; a segment's output is one contiguous range.
// pass 2 (smi_dedup_emit_segment), per segment, the same bytes again:
//   K-DD-WRITE: one wavefront per record of the segment, the ones that lost leave at once.  Lane 0 writes the marker, the separators and
//     the decimal rn; all lanes copy ids[0], ids[1] (from the pool), the sequence and the quality line: bytes up to the destination's
//     next 4-byte boundary, then dwords, then the tail.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "smi_device.h"
#include "smi_internal.h"

namespace smi {
namespace {

constexpr int kDdBlock = 256;
constexpr int kDdWaves = 4;  // waves per block of K-DD-WRITE
constexpr uint64_t kNone = ~0ull;
// transition functions, next state of state s in bits 2s+1 .. 2s: a marker line (0 -> 1) and any other line (0 -> 0); 1 -> 2 -> 3 -> 0 for both
constexpr uint8_t kFqMarker = 0x39, kFqOther = 0x38, kFaMarker = 0x01, kFaOther = 0x00;

constexpr const char *kWho = "DeduplicateMolecule";  // the program named when a device allocation fails

// a device array that keeps its contents when it grows (the key pool and the record table live across segments)
template <class T>
struct Grow {
    T *p = nullptr;
    size_t cap = 0;
    Grow() = default;
    Grow(const Grow &) = delete;
    ~Grow() {
        if (p) (void)hipFree(p);
    }
    int reserve(size_t n, size_t keep, hipStream_t s) {
        if (n <= cap) return SMI_OK;
        const size_t nc = std::max<size_t>(std::max(n, cap * 2), 4096);
        T *q = nullptr;
        if (hipMalloc((void **)&q, nc * sizeof(T)) != hipSuccess) {
            set_error("DeduplicateMolecule: device allocation of " + std::to_string(nc * sizeof(T)) + " bytes failed");
            return SMI_ERR_HIP;
        }
        if (keep) {
            SMI_HIP(hipMemcpyAsync(q, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s));
            SMI_HIP(hipStreamSynchronize(s));
        }
        if (p) (void)hipFree(p);
        p = q;
        cap = nc;
        return SMI_OK;
    }
};

struct DdRec {
    uint64_t pool_off, hash;        // ids[0] + ids[1] at pool[pool_off ..+ key_len), ids[0] = the first len0 bytes
    uint64_t seq_start, qual_start; // in the segment's text
    uint32_t key_len, len0, seq_len, qual_len;
    int32_t rn;
    uint32_t pad;
};

// what one segment reports back
struct DdSeg {
    uint64_t incomplete_line;  // the record start whose lines are not all inside a segment that is not the last, or kNone
    uint64_t err_line;         // the smallest offending line, 1-based over the whole input, or kNone
    uint64_t n_null, n_skipped;
};

struct Compose {  // a, then b
    __host__ __device__ uint8_t operator()(uint8_t a, uint8_t b) const {
        uint32_t r = 0;
#pragma unroll
        for (int s = 0; s < 4; s++) r |= ((b >> (2 * ((a >> (2 * s)) & 3))) & 3u) << (2 * s);
        return (uint8_t)r;
    }
};

// one past the last byte of line L: the LF dropped, and one CR in front of it
__device__ __forceinline__ uint64_t line_end(const uint8_t *__restrict__ text, const uint64_t *__restrict__ line_start, uint64_t L) {
    const uint64_t b = line_start[L];
    uint64_t e = line_start[L + 1] - 1;
    if (e > b && text[e - 1] == '\r') e--;
    return e;
}

__global__ __launch_bounds__(kDdBlock) void k_dd_func(const uint8_t *__restrict__ text, const uint64_t *__restrict__ line_start, uint64_t n_lines,
                                                      uint64_t line_base, int fasta, uint8_t *__restrict__ f, DdSeg *__restrict__ seg) {
    const uint64_t L = blockIdx.x * (uint64_t)kDdBlock + threadIdx.x;
    if (L >= n_lines) return;
    const uint64_t b = line_start[L], e = line_start[L + 1] - 1;
    const bool m = e > b && text[b] == (fasta ? '>' : '@');
    f[L] = fasta ? (m ? kFaMarker : kFaOther) : (m ? kFqMarker : kFqOther);
    if (e - b >= (1ull << 32)) atomicMin((unsigned long long *)&seg->err_line, (unsigned long long)(line_base + L + 1));
}

// flag[L] = 1 where a record starts; lines met outside a record that start none are the skipped ones
__global__ __launch_bounds__(kDdBlock) void k_dd_flag(const uint8_t *__restrict__ f, const uint8_t *__restrict__ fs, uint64_t n_lines,
                                                      uint32_t *__restrict__ flag, DdSeg *__restrict__ seg) {
    const uint64_t L = blockIdx.x * (uint64_t)kDdBlock + threadIdx.x;
    bool start = false, skip = false;
    if (L < n_lines) {
        const uint32_t state = L ? (fs[L - 1] & 3u) : 0u;
        const bool m = (f[L] & 3u) == 1u;  // both marker functions send state 0 to 1
        start = state == 0 && m;
        skip = state == 0 && !m;
        flag[L] = start;
    } else if (L == n_lines) {
        flag[L] = 0;
    }
    const unsigned long long bal = __ballot(skip);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd((unsigned long long *)&seg->n_skipped, (unsigned long long)__popcll(bal));
}

__global__ __launch_bounds__(kDdBlock) void k_dd_starts(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ ridx, uint64_t n_lines,
                                                        uint64_t *__restrict__ start_line) {
    const uint64_t L = blockIdx.x * (uint64_t)kDdBlock + threadIdx.x;
    if (L < n_lines && flag[L]) start_line[ridx[L]] = L;
}

struct Name {
    uint32_t len0, len1;
    int32_t rn;
    uint64_t hash;
    bool ok;
};

// L202-206 over the header's bytes in one walk: every marker byte removed, then backslash + '|' -> '-' (String.replace: literal, left to
// right), then split("-"): ids[0], ids[1], ids[2].  Trailing empty fields do not exist for split, so an empty ids[2] is either no third
// field or no number: an error both ways.  rn = Integer(ids[2]): an optional '+', decimal digits, at most 2147483647.
template <bool WRITE>
__device__ Name parse_name(const uint8_t *__restrict__ p, uint32_t n, uint8_t marker, uint8_t *__restrict__ key) {
    Name o = {0, 0, 0, kFnvBasis, false};
    uint32_t i = 0, field = 0, nd = 0, k = 0, at = 0;
    uint64_t v = 0;
    bool bad = false;
    while (field < 3) {
        while (i < n && p[i] == marker) i++;
        if (i >= n) break;
        uint8_t c = p[i++];
        if (c == '\\') {
            uint32_t j = i;
            while (j < n && p[j] == marker) j++;
            if (j < n && p[j] == '|') {
                i = j + 1;
                c = '-';
            }
        }
        if (c == '-') {
            field++;
            continue;
        }
        if (field < 2) {
            o.hash = fnv1a_add(o.hash, c);
            if (WRITE) key[k] = c;
            k++;
            if (field == 0) o.len0++;
            else o.len1++;
        } else {
            if (c >= '0' && c <= '9') {
                v = v * 10 + (c - '0');
                if (v > 2147483647ull) {
                    bad = true;
                    v = 0;
                }
                nd++;
            } else if (!(c == '+' && at == 0)) {
                bad = true;
            }
            at++;
        }
    }
    o.rn = (int32_t)v;
    o.ok = field >= 2 && nd > 0 && !bad;
    return o;
}

struct ParseArgs {
    const uint8_t *text;
    const uint64_t *line_start, *start_line;
    uint64_t n_lines, n_starts, line_base;
    int fasta, is_last;
    DdSeg *seg;
    uint32_t *valid;        // COUNT: 1 for a record that is kept; WRITE: its exclusive scan
    uint64_t *klen;         // COUNT: its key bytes; WRITE: their exclusive scan
    DdRec *recs;            // WRITE: at the handle's record count
    uint8_t *pool;          // WRITE: at the handle's pool size
    uint64_t pool_base;
};

template <bool WRITE>
__global__ __launch_bounds__(kDdBlock) void k_dd_parse(ParseArgs a) {
    const uint64_t r = blockIdx.x * (uint64_t)kDdBlock + threadIdx.x;
    if (r >= a.n_starts) return;
    const uint64_t L = a.start_line[r];
    const uint64_t avail = a.n_lines - L, need = a.fasta ? 2 : 4;
    const uint8_t marker = a.fasta ? '>' : '@';
    bool keep = false;
    uint64_t kl = 0;
    if (avail < need && !a.is_last) {
        if (!WRITE) a.seg->incomplete_line = L;  // at most one: every line behind it is inside it
    } else {
        bool is_null = false;
        uint64_t sb = 0, se = 0;
        if (avail >= 2) {
            sb = a.line_start[L + 1];
            se = line_end(a.text, a.line_start, L + 1);
            is_null = se - sb == 4 && a.text[sb] == 'n' && a.text[sb + 1] == 'u' && a.text[sb + 2] == 'l' && a.text[sb + 3] == 'l';
        }
        if (is_null) {  // L192 / L118: dropped and not counted, before anything else of it is looked at
            if (!WRITE) atomicAdd((unsigned long long *)&a.seg->n_null, 1ull);
        } else if (avail < need) {  // cut short by the end of the input
            if (!WRITE) atomicMin((unsigned long long *)&a.seg->err_line, (unsigned long long)(a.line_base + L + 1));
        } else {
            const uint64_t hb = a.line_start[L], he = line_end(a.text, a.line_start, L);
            if (!WRITE) {
                const Name nm = parse_name<false>(a.text + hb, (uint32_t)(he - hb), marker, nullptr);
                if (nm.ok) {
                    keep = true;
                    kl = (uint64_t)nm.len0 + nm.len1;
                } else {
                    atomicMin((unsigned long long *)&a.seg->err_line, (unsigned long long)(a.line_base + L + 1));
                }
            } else if (a.valid[r + 1] != a.valid[r]) {
                const uint64_t po = a.pool_base + a.klen[r];
                const Name nm = parse_name<true>(a.text + hb, (uint32_t)(he - hb), marker, a.pool + po);
                DdRec o;
                o.pool_off = po;
                o.hash = nm.hash;
                o.seq_start = sb;
                o.seq_len = (uint32_t)(se - sb);
                o.qual_start = 0;
                o.qual_len = 0;
                if (!a.fasta) {
                    o.qual_start = a.line_start[L + 3];
                    o.qual_len = (uint32_t)(line_end(a.text, a.line_start, L + 3) - o.qual_start);
                }
                o.key_len = nm.len0 + nm.len1;
                o.len0 = nm.len0;
                o.rn = nm.rn;
                o.pad = 0;
                a.recs[a.valid[r]] = o;
            }
        }
    }
    if (!WRITE) {
        a.valid[r] = keep;
        a.klen[r] = kl;
    }
}

struct TabArgs {
    const DdRec *recs;
    const uint8_t *pool;
    uint32_t n, mask;
    uint64_t hash_mask;
    uint32_t *tab, *group;
    unsigned long long *probe_steps, *wraps;
};

__global__ __launch_bounds__(kDdBlock) void k_dd_insert(TabArgs a) {
    const uint32_t i = blockIdx.x * kDdBlock + threadIdx.x;
    if (i >= a.n) return;
    const DdRec r = a.recs[i];
    const DdRec *recs = a.recs;
    const uint8_t *pool = a.pool;
    // (the table has two slots per record: the walk always ends at an entry)
    const Probed p = probe<true>(a.tab, a.mask, (uint32_t)(r.hash & a.hash_mask) & a.mask, i, Bytes{pool + r.pool_off, r.key_len},
                                 [recs, pool](uint32_t e) { return Bytes{pool + recs[e].pool_off, recs[e].key_len}; });
    a.group[i] = p.entry;
    if (p.steps) atomicAdd(a.probe_steps, (unsigned long long)p.steps);
    if (p.wraps) atomicAdd(a.wraps, (unsigned long long)p.wraps);
}

enum : int { kModeSelect = 0, kModeFasta = 1, kModeFirst = 2 };

struct PickArgs {
    const DdRec *recs;
    const uint32_t *group;
    uint32_t n;
    int mode;
    unsigned long long *best;  // per representative
    uint32_t *win, *last_ne;   // smallest index; FASTA: 1 + the largest index with a non-empty sequence, 0 = none
    uint64_t *size;            // n + 1
    unsigned long long *n_mol;
};

__device__ __forceinline__ unsigned long long pick_key(const DdRec &r, int mode) {
    return (unsigned long long)(uint32_t)r.rn << 32 | (mode == kModeSelect ? r.seq_len : 0u);
}

__global__ __launch_bounds__(kDdBlock) void k_dd_pick_max(PickArgs a) {
    const uint32_t i = blockIdx.x * kDdBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t g = a.group[i];
    if (a.mode == kModeFirst) atomicMin(&a.win[g], i);
    else atomicMax(&a.best[g], pick_key(a.recs[i], a.mode));
}

__global__ __launch_bounds__(kDdBlock) void k_dd_pick_index(PickArgs a) {
    const uint32_t i = blockIdx.x * kDdBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t g = a.group[i];
    const DdRec &r = a.recs[i];
    if (pick_key(r, a.mode) != a.best[g]) return;
    atomicMin(&a.win[g], i);
    if (a.mode == kModeFasta && r.seq_len > 0) atomicMax(&a.last_ne[g], i + 1);
}

// size[i]: bytes of record i in the output, 0 when it is not its molecule's winner
__global__ __launch_bounds__(kDdBlock) void k_dd_size(PickArgs a) {
    const uint32_t i = blockIdx.x * kDdBlock + threadIdx.x;
    bool won = false;
    if (i < a.n) {
        const uint32_t g = a.group[i];
        uint32_t w = a.win[g];
        if (a.mode == kModeFasta && a.last_ne[g]) w = a.last_ne[g] - 1;
        won = w == i;
        uint64_t sz = 0;
        if (won) {
            const DdRec &r = a.recs[i];
            sz = 1 + (uint64_t)r.key_len + 2 + digits((uint32_t)r.rn) + 1 + r.seq_len + 1;  // marker ids0 - ids1 - rn \n seq \n
            if (a.mode != kModeFasta) sz += 2 + (uint64_t)r.qual_len + 1;                       // + \n qual \n
        }
        a.size[i] = sz;
    } else if (i == a.n) {
        a.size[i] = 0;
    }
    const unsigned long long bal = __ballot(won);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(a.n_mol, (unsigned long long)__popcll(bal));
}

__global__ __launch_bounds__(64 * kDdWaves) void k_dd_write(const uint8_t *__restrict__ text, const DdRec *__restrict__ recs,
                                                            const uint64_t *__restrict__ out_off, const uint8_t *__restrict__ pool, uint32_t rec0,
                                                            uint32_t n, int fasta, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint32_t w = blockIdx.x * kDdWaves + (threadIdx.x >> 6);
    if (w >= n) return;
    const uint32_t i = rec0 + w;
    const uint64_t o = out_off[i];
    if (out_off[i + 1] == o) return;
    const DdRec r = recs[i];
    uint8_t *dst = out + (o - out_off[rec0]);
    const uint32_t len1 = r.key_len - r.len0;
    const int nd = digits((uint32_t)r.rn);
    uint8_t *num = dst + 1 + r.len0 + 1 + len1 + 1, *seq = num + nd + 1, *qual = seq + r.seq_len + 3;
    if (lane == 0) {
        dst[0] = fasta ? '>' : '@';
        dst[1 + r.len0] = '-';
        num[-1] = '-';
        uint32_t v = (uint32_t)r.rn;
        for (int k = nd - 1; k >= 0; k--) {
            num[k] = (uint8_t)('0' + v % 10);
            v /= 10;
        }
        num[nd] = '\n';
        seq[r.seq_len] = '\n';
        if (!fasta) {
            seq[r.seq_len + 1] = '+';
            seq[r.seq_len + 2] = '\n';
            qual[r.qual_len] = '\n';
        }
    }
    wave_copy(dst + 1, pool + r.pool_off, r.len0, lane);
    wave_copy(dst + 2 + r.len0, pool + r.pool_off + r.len0, len1, lane);
    wave_copy(seq, text + r.seq_start, r.seq_len, lane);
    if (!fasta) wave_copy(qual, text + r.qual_start, r.qual_len, lane);
}

struct Segment {
    uint64_t consumed;
    uint32_t rec0, n_rec;
};

}  // namespace
}  // namespace smi

using namespace smi;

struct smi_dedup {
    smi_ctx *ctx = nullptr;
    smi_dedup_config cfg = {};
    Grow<uint8_t> pool, d_text;
    Grow<DdRec> recs;
    DevBuf<uint64_t> d_out_off{kWho};
    uint64_t pool_bytes = 0, n_rec = 0, line_base = 0, err_line = 0;
    std::vector<Segment> segs;
    bool last_seen = false, selected = false;
    int64_t counts[SMI_DEDUP_COUNTS] = {};
    float ms[SMI_DEDUP_STAGES] = {};
};

extern "C" int smi_dedup_default_config(smi_dedup_config *cfg) {
    if (!cfg) {
        set_error("smi_dedup_default_config: null argument");
        return SMI_ERR_INVALID;
    }
    *cfg = {};
    cfg->fasta = 0;
    cfg->select = 1;
    cfg->hash_bits = 64;
    cfg->min_table_slots = 0;
    return SMI_OK;
}

extern "C" int smi_dedup_create(smi_ctx *ctx, const smi_dedup_config *cfg, smi_dedup **out) {
    if (!ctx || !cfg || !out) {
        set_error("smi_dedup_create: null argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    if (cfg->hash_bits < 0 || cfg->hash_bits > 64) {
        set_error("smi_dedup_create: hash_bits " + std::to_string(cfg->hash_bits) + " outside 0 .. 64");
        return SMI_ERR_INVALID;
    }
    if (cfg->min_table_slots < 0 || cfg->min_table_slots > (int64_t)1 << 32) {
        set_error("smi_dedup_create: min_table_slots " + std::to_string(cfg->min_table_slots) + " outside 0 .. 2^32");
        return SMI_ERR_INVALID;
    }
    std::unique_ptr<smi_dedup> h(new smi_dedup());
    h->ctx = ctx;
    h->cfg = *cfg;
    *out = h.release();
    return SMI_OK;
}

extern "C" int smi_dedup_free(smi_dedup *h) {
    delete h;
    return SMI_OK;
}

extern "C" int smi_dedup_add_segment(smi_dedup *h, const uint8_t *text, size_t n_bytes, int32_t is_last, size_t *consumed) {
    if (!h || !consumed || (n_bytes && !text)) {
        set_error("smi_dedup_add_segment: null argument");
        return SMI_ERR_INVALID;
    }
    *consumed = 0;
    if (h->last_seen || h->selected || h->err_line) {
        set_error("smi_dedup_add_segment: the input was already closed (a last segment, an error or smi_dedup_select)");
        return SMI_ERR_STATE;
    }
    const bool fasta = h->cfg.fasta != 0, last = is_last != 0;
    const bool open_end = n_bytes && text[n_bytes - 1] != '\n';  // bytes behind the last LF: a line only at the end of the input
    Segment sg = {0, (uint32_t)h->n_rec, 0};
    uint64_t lines_used = 0;
    DdSeg res = {kNone, kNone, 0, 0};
    const uint64_t behind = (uint64_t)n_bytes + 1;
    if (n_bytes) {
        SMI_HIP(hipSetDevice(h->ctx->device));
        hipStream_t s = h->ctx->stream;
        int rc;
        if ((rc = h->d_text.reserve(n_bytes, 0, s))) return rc;
        SMI_HIP(hipMemcpyAsync(h->d_text.p, text, n_bytes, hipMemcpyHostToDevice, s));
        Events ev;
        if ((rc = ev.begin(s))) return rc;
        size_t swept_lines = 0;
        if ((rc = launch_fastq_sweep(h->ctx, h->d_text.p, n_bytes, &swept_lines, s))) return rc;
        const uint64_t n_nl = swept_lines - (open_end ? 1 : 0);
        const uint64_t n_lines = n_nl + (open_end && last ? 1 : 0);
        if (n_lines >= (uint64_t)INT32_MAX - 1) {
            set_error("DeduplicateMolecule: " + std::to_string(n_lines) + " lines in one segment; at most 2^31 - 3 are indexed at once: pass smaller segments");
            return SMI_ERR_INVALID;
        }
        if (n_lines) {
            DevBuf<uint64_t> d_line{kWho}, d_start{kWho}, d_klen{kWho}, d_koff{kWho};
            DevBuf<uint8_t> d_f{kWho}, d_fs{kWho};
            Scratch tmp{kWho};
            DevBuf<uint32_t> d_flag{kWho}, d_ridx{kWho}, d_valid{kWho}, d_vidx{kWho};
            DevBuf<DdSeg> d_seg{kWho};
            if ((rc = d_line.alloc(n_lines + 1)) || (rc = d_f.alloc(n_lines)) || (rc = d_fs.alloc(n_lines)) || (rc = d_flag.alloc(n_lines + 1)) ||
                (rc = d_ridx.alloc(n_lines + 1)) || (rc = d_seg.alloc(1)))
                return rc;
            SMI_HIP(hipMemcpyAsync(d_seg.p, &res, sizeof res, hipMemcpyHostToDevice, s));
            // entries 0 .. n_nl come from the sweep; a last line without LF ends as if one stood behind the text
            if ((rc = launch_fastq_line_starts(h->ctx, h->d_text.p, n_bytes, d_line.p, (size_t)n_nl + 1, s))) return rc;
            if (n_lines > n_nl) SMI_HIP(hipMemcpyAsync(d_line.p + n_lines, &behind, 8, hipMemcpyHostToDevice, s));
            const unsigned grid_l = (unsigned)((n_lines + 1 + kDdBlock - 1) / kDdBlock);
            hipLaunchKernelGGL(k_dd_func, dim3(grid_l), dim3(kDdBlock), 0, s, (const uint8_t *)h->d_text.p, (const uint64_t *)d_line.p, n_lines, h->line_base,
                               (int)fasta, d_f.p, d_seg.p);
            SMI_HIP(hipGetLastError());
            const auto compose = [&](void *p, size_t &t) { return hipcub::DeviceScan::InclusiveScan(p, t, d_f.p, d_fs.p, Compose(), (int)n_lines, s); };
            const auto sum = [s](auto *in, auto *out, size_t m) {
                return [=](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, in, out, (int)m, s); };
            };
            const auto flags = sum(d_flag.p, d_ridx.p, n_lines + 1);
            if ((rc = reserve(tmp, compose, flags))) return rc;
            if ((rc = run_reserved(tmp, compose))) return rc;
            hipLaunchKernelGGL(k_dd_flag, dim3(grid_l), dim3(kDdBlock), 0, s, (const uint8_t *)d_f.p, (const uint8_t *)d_fs.p, n_lines, d_flag.p, d_seg.p);
            SMI_HIP(hipGetLastError());
            if ((rc = run_reserved(tmp, flags))) return rc;
            uint32_t n_starts = 0;
            SMI_HIP(hipMemcpyAsync(&n_starts, d_ridx.p + n_lines, 4, hipMemcpyDeviceToHost, s));
            if ((rc = ev.end(s, &h->ms[SMI_DEDUP_MS_INDEX]))) return rc;
            if (n_starts) {
                if ((rc = d_start.alloc(n_starts)) || (rc = d_valid.alloc((size_t)n_starts + 1)) || (rc = d_vidx.alloc((size_t)n_starts + 1)) ||
                    (rc = d_klen.alloc((size_t)n_starts + 1)) || (rc = d_koff.alloc((size_t)n_starts + 1)))
                    return rc;
                const auto valid = sum(d_valid.p, d_vidx.p, (size_t)n_starts + 1);
                const auto keys = sum(d_klen.p, d_koff.p, (size_t)n_starts + 1);
                if ((rc = reserve(tmp, valid, keys))) return rc;
                if ((rc = ev.begin(s))) return rc;
                hipLaunchKernelGGL(k_dd_starts, dim3(grid_l), dim3(kDdBlock), 0, s, (const uint32_t *)d_flag.p, (const uint32_t *)d_ridx.p, n_lines, d_start.p);
                SMI_HIP(hipMemsetAsync(d_valid.p + n_starts, 0, 4, s));
                SMI_HIP(hipMemsetAsync(d_klen.p + n_starts, 0, 8, s));
                ParseArgs a = {};
                a.text = h->d_text.p;
                a.line_start = d_line.p;
                a.start_line = d_start.p;
                a.n_lines = n_lines;
                a.n_starts = n_starts;
                a.line_base = h->line_base;
                a.fasta = fasta;
                a.is_last = last;
                a.seg = d_seg.p;
                a.valid = d_valid.p;
                a.klen = d_klen.p;
                const unsigned grid_r = (n_starts + kDdBlock - 1) / kDdBlock;
                hipLaunchKernelGGL(k_dd_parse<false>, dim3(grid_r), dim3(kDdBlock), 0, s, a);
                SMI_HIP(hipGetLastError());
                if ((rc = run_reserved(tmp, valid)) || (rc = run_reserved(tmp, keys))) return rc;
                uint32_t n_valid = 0;
                uint64_t key_bytes = 0;
                SMI_HIP(hipMemcpyAsync(&n_valid, d_vidx.p + n_starts, 4, hipMemcpyDeviceToHost, s));
                SMI_HIP(hipMemcpyAsync(&key_bytes, d_koff.p + n_starts, 8, hipMemcpyDeviceToHost, s));
                SMI_HIP(hipMemcpyAsync(&res, d_seg.p, sizeof res, hipMemcpyDeviceToHost, s));
                SMI_HIP(hipStreamSynchronize(s));
                if (res.err_line == kNone && n_valid) {
                    if (h->n_rec + n_valid >= (uint64_t)INT32_MAX - 1) {
                        set_error("DeduplicateMolecule: more than 2^31 - 3 records; the molecule table indexes them with 32 bits");
                        return SMI_ERR_INVALID;
                    }
                    if ((rc = h->recs.reserve(h->n_rec + n_valid, h->n_rec, s)) || (rc = h->pool.reserve(h->pool_bytes + key_bytes, h->pool_bytes, s))) return rc;
                    a.valid = d_vidx.p;
                    a.klen = d_koff.p;
                    a.recs = h->recs.p + h->n_rec;
                    a.pool = h->pool.p;
                    a.pool_base = h->pool_bytes;
                    hipLaunchKernelGGL(k_dd_parse<true>, dim3(grid_r), dim3(kDdBlock), 0, s, a);
                    SMI_HIP(hipGetLastError());
                }
                if ((rc = ev.end(s, &h->ms[SMI_DEDUP_MS_PARSE]))) return rc;
                if (res.err_line == kNone) {
                    sg.n_rec = n_valid;
                    h->pool_bytes += key_bytes;
                }
            } else {
                SMI_HIP(hipMemcpyAsync(&res, d_seg.p, sizeof res, hipMemcpyDeviceToHost, s));
                SMI_HIP(hipStreamSynchronize(s));
            }
            if (res.err_line != kNone) {
                h->err_line = res.err_line;
                set_error("DeduplicateMolecule: line " + std::to_string(res.err_line) +
                          ": a line of 2^32 bytes or more, a record cut short by the end of the input, or a name without three '-' separated fields "
                          "whose third is an integer");
                return SMI_ERR_INVALID;
            }
            lines_used = res.incomplete_line != kNone ? res.incomplete_line : n_lines;
            uint64_t used_bytes = n_bytes;
            if (!(last && lines_used == n_lines)) SMI_HIP(hipMemcpy(&used_bytes, d_line.p + lines_used, 8, hipMemcpyDeviceToHost));
            sg.consumed = used_bytes;
        } else {
            h->ctx->fq_swept_text = nullptr;  // the sweep's flags are not used: nothing may take them for another text's
            sg.consumed = last ? n_bytes : 0;
        }
    }
    if (!last && sg.consumed == 0) return SMI_OK;  // no whole record or skipped line in it: the caller comes again with more bytes
    h->n_rec += sg.n_rec;
    h->line_base += lines_used;
    h->counts[SMI_DEDUP_LINES] += (int64_t)lines_used;
    h->counts[SMI_DEDUP_RECORDS] += sg.n_rec;
    h->counts[SMI_DEDUP_NULL] += (int64_t)res.n_null;
    h->counts[SMI_DEDUP_SKIPPED] += (int64_t)res.n_skipped;
    h->counts[SMI_DEDUP_SEGMENTS]++;
    h->segs.push_back(sg);
    h->last_seen = last;
    *consumed = (size_t)sg.consumed;
    return SMI_OK;
}

extern "C" int smi_dedup_select(smi_dedup *h, float *stage_ms) {
    if (!h) {
        set_error("smi_dedup_select: null argument");
        return SMI_ERR_INVALID;
    }
    if (!h->last_seen || h->selected) {
        set_error(h->selected ? "smi_dedup_select: already run" : "smi_dedup_select: the last segment has not been added");
        return SMI_ERR_STATE;
    }
    h->selected = true;
    const uint32_t n = (uint32_t)h->n_rec;
    uint64_t slots = 2;
    while (slots < 2 * (uint64_t)n || slots < (uint64_t)h->cfg.min_table_slots) slots <<= 1;
    h->counts[SMI_DEDUP_TABLE_SLOTS] = (int64_t)slots;
    if (n) {
        SMI_HIP(hipSetDevice(h->ctx->device));
        hipStream_t s = h->ctx->stream;
        DevBuf<uint32_t> d_tab{kWho}, d_group{kWho}, d_win{kWho}, d_last{kWho};
        DevBuf<unsigned long long> d_best{kWho}, d_cnt{kWho};
        DevBuf<uint64_t> d_size{kWho};
        Scratch tmp{kWho};
        int rc;
        if ((rc = d_tab.alloc(slots)) || (rc = d_group.alloc(n)) || (rc = d_win.alloc(n)) || (rc = d_last.alloc(n)) || (rc = d_best.alloc(n)) ||
            (rc = d_cnt.alloc(3)) || (rc = d_size.alloc((size_t)n + 1)) || (rc = h->d_out_off.alloc((size_t)n + 1)))
            return rc;
        const auto offsets = [&](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, d_size.p, h->d_out_off.p, (int)n + 1, s); };
        if ((rc = reserve(tmp, offsets))) return rc;
        SMI_HIP(hipMemsetAsync(d_tab.p, 0xff, slots * 4, s));
        SMI_HIP(hipMemsetAsync(d_win.p, 0xff, (size_t)n * 4, s));
        SMI_HIP(hipMemsetAsync(d_last.p, 0, (size_t)n * 4, s));
        SMI_HIP(hipMemsetAsync(d_best.p, 0, (size_t)n * 8, s));
        SMI_HIP(hipMemsetAsync(d_cnt.p, 0, 3 * 8, s));
        const unsigned grid = (n + kDdBlock - 1) / kDdBlock, grid1 = n / kDdBlock + 1;
        Events ev;
        if ((rc = ev.begin(s))) return rc;
        TabArgs t = {};
        t.recs = h->recs.p;
        t.pool = h->pool.p;
        t.n = n;
        t.mask = (uint32_t)(slots - 1);
        t.hash_mask = h->cfg.hash_bits >= 64 ? ~0ull : ((1ull << h->cfg.hash_bits) - 1);
        t.tab = d_tab.p;
        t.group = d_group.p;
        t.probe_steps = d_cnt.p;
        t.wraps = d_cnt.p + 1;
        hipLaunchKernelGGL(k_dd_insert, dim3(grid), dim3(kDdBlock), 0, s, t);
        SMI_HIP(hipGetLastError());
        if ((rc = ev.end(s, &h->ms[SMI_DEDUP_MS_INSERT]))) return rc;
        if ((rc = ev.begin(s))) return rc;
        PickArgs p = {};
        p.recs = h->recs.p;
        p.group = d_group.p;
        p.n = n;
        p.mode = h->cfg.fasta ? kModeFasta : h->cfg.select ? kModeSelect : kModeFirst;
        p.best = d_best.p;
        p.win = d_win.p;
        p.last_ne = d_last.p;
        p.size = d_size.p;
        p.n_mol = d_cnt.p + 2;
        hipLaunchKernelGGL(k_dd_pick_max, dim3(grid), dim3(kDdBlock), 0, s, p);
        if (p.mode != kModeFirst) hipLaunchKernelGGL(k_dd_pick_index, dim3(grid), dim3(kDdBlock), 0, s, p);
        hipLaunchKernelGGL(k_dd_size, dim3(grid1), dim3(kDdBlock), 0, s, p);
        SMI_HIP(hipGetLastError());
        if ((rc = run_reserved(tmp, offsets))) return rc;
        if ((rc = ev.end(s, &h->ms[SMI_DEDUP_MS_PICK]))) return rc;
        unsigned long long cnt[3] = {0, 0, 0};
        uint64_t total = 0;
        SMI_HIP(hipMemcpy(cnt, d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost));
        SMI_HIP(hipMemcpy(&total, h->d_out_off.p + n, 8, hipMemcpyDeviceToHost));
        h->counts[SMI_DEDUP_PROBE_STEPS] = (int64_t)cnt[0];
        h->counts[SMI_DEDUP_WRAPS] = (int64_t)cnt[1];
        h->counts[SMI_DEDUP_MOLECULES] = (int64_t)cnt[2];
        h->counts[SMI_DEDUP_BYTES] = (int64_t)total;
    }
    if (stage_ms) std::memcpy(stage_ms, h->ms, sizeof(h->ms));
    return SMI_OK;
}

extern "C" int smi_dedup_emit_segment(smi_dedup *h, int32_t segment, const uint8_t *text, size_t n_bytes, uint8_t *out, size_t cap, size_t *n_out) {
    if (!h || !n_out) {
        set_error("smi_dedup_emit_segment: null argument");
        return SMI_ERR_INVALID;
    }
    *n_out = 0;
    if (!h->selected) {
        set_error("smi_dedup_emit_segment: smi_dedup_select has not run");
        return SMI_ERR_STATE;
    }
    if (segment < 0 || (size_t)segment >= h->segs.size()) {
        set_error("smi_dedup_emit_segment: segment " + std::to_string(segment) + " of " + std::to_string(h->segs.size()));
        return SMI_ERR_INVALID;
    }
    const Segment &sg = h->segs[segment];
    if (sg.n_rec == 0) return SMI_OK;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    uint64_t range[2] = {0, 0};
    SMI_HIP(hipMemcpy(&range[0], h->d_out_off.p + sg.rec0, 8, hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(&range[1], h->d_out_off.p + sg.rec0 + sg.n_rec, 8, hipMemcpyDeviceToHost));
    const uint64_t size = range[1] - range[0];
    *n_out = (size_t)size;
    if (!out) return SMI_OK;
    if (cap < size) return 1;
    if (!size) return SMI_OK;
    if (!text || n_bytes < sg.consumed) {
        set_error("smi_dedup_emit_segment: segment " + std::to_string(segment) + " had " + std::to_string(sg.consumed) + " bytes in pass 1, " +
                  std::to_string(n_bytes) + " are passed now");
        return SMI_ERR_INVALID;
    }
    int rc;
    DevBuf<uint8_t> d_out{kWho};
    if ((rc = h->d_text.reserve(sg.consumed, 0, s)) || (rc = d_out.alloc(size))) return rc;
    SMI_HIP(hipMemcpyAsync(h->d_text.p, text, sg.consumed, hipMemcpyHostToDevice, s));
    Events ev;
    if ((rc = ev.begin(s))) return rc;
    hipLaunchKernelGGL(k_dd_write, dim3((sg.n_rec + kDdWaves - 1) / kDdWaves), dim3(64 * kDdWaves), 0, s, (const uint8_t *)h->d_text.p, (const DdRec *)h->recs.p,
                       (const uint64_t *)h->d_out_off.p, (const uint8_t *)h->pool.p, sg.rec0, sg.n_rec, (int)(h->cfg.fasta != 0), d_out.p);
    SMI_HIP(hipGetLastError());
    if ((rc = ev.end(s, &h->ms[SMI_DEDUP_MS_WRITE]))) return rc;
    SMI_HIP(hipMemcpy(out, d_out.p, size, hipMemcpyDeviceToHost));
    return SMI_OK;
}

extern "C" int smi_dedup_counts(const smi_dedup *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_dedup_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof(h->counts));
    return SMI_OK;
}

extern "C" int smi_dedup_stage_ms(const smi_dedup *h, float *stage_ms) {
    if (!h || !stage_ms) {
        set_error("smi_dedup_stage_ms: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(stage_ms, h->ms, sizeof(h->ms));
    return SMI_OK;
}

extern "C" int smi_dedup_error_line(const smi_dedup *h, int64_t *line) {
    if (!h || !line) {
        set_error("smi_dedup_error_line: null argument");
        return SMI_ERR_INVALID;
    }
    *line = (int64_t)h->err_line;
    return SMI_OK;
}
