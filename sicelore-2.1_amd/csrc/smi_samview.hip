// smi_samview.hip -- `SamView`: SAM text to BAM records, in the place of `samtools view -bS`.  The conversion is this build's own canonical
// definition (tests/sammodel.py restates it).  No byte equality with `samtools view` is claimed.
//
// The host turns the header lines into the BAM header and a table of the @SQ names (smi_samview_create); the alignment lines come in
// segments that end on a line end (smi_samview_add_segment).  Per segment
//   line table   K-FQ's sweep through launch_fastq_sweep / launch_fastq_line_starts (smi_fastq.hip)
//   K-SAM-SIZE   one wavefront per line: the first eleven tabs by ballots over 4-byte loads, the numeric fields and the two reference
//                names one lane each, the CIGAR operations and the attributes one lane each in strides; every rule of the definition is
//                checked here (the first bad line is kept by atomicMin), the fixed 36 bytes and the field borders go to a per-line entry,
//                the record's byte length to the scan
//   hipcub       exclusive sum of the lengths: every record's offset and the total
//   K-SAM-WRITE  one wavefront per line again: the fixed bytes, the name, the CIGAR words, SEQ packed eight bases to an aligned 32-bit
//                word per lane, QUAL four bytes to an aligned word per lane, the attributes behind a prefix sum of their sizes
// and the library's BGZF deflater (smi_bgzf_deflate_device) on the record buffer (smi_samview_convert).
// No lane loops over the bytes of SEQ or QUAL; a lane does loop over the bytes of its own number, reference name, CIGAR length or
// attribute.  Every load lies inside the line, every store inside the record.
#include <chrono>
#include <climits>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "smi_auxedit.h"
#include "smi_handle.h"

#define SV_HD __host__ __device__ __forceinline__

namespace smi {
namespace {

constexpr int kSvBlock = 256;
constexpr int kSvWaves = kSvBlock / 64;  // lines per block (why a wavefront per line)
constexpr uint32_t kSvStep = 256;        // bytes of a line a wavefront looks at per step: 4 per lane
constexpr unsigned long long kNoStop = ~0ull;
constexpr uint64_t kSvMaxSegment = 1ull << 31;  // a segment's bytes and lines are counted in 32 bits

// why a line stops the run, in the order the rules are listed; a line that breaks several is named with the first of them
enum : uint32_t {
    kSvLate = 1, kSvFields, kSvName, kSvFlag, kSvRname, kSvPos, kSvMapq, kSvCigar, kSvCigarMany, kSvRnext, kSvPnext, kSvTlen, kSvQualLen,
    kSvAttr, kSvAttrInt, kSvAttrFloat, kSvAttrB, kSvNone = 63
};
const char *const kSvReason[] = {
    "",
    "a header line behind the first alignment line",
    "fewer than 11 fields",
    "the read name is empty or longer than 254 bytes",
    "FLAG is not a number in 0 .. 65535",
    "RNAME is not * or one of the header's references",
    "POS is not a number in 0 .. 2^31 - 1",
    "MAPQ is not a number in 0 .. 255",
    "CIGAR is not * or operations of MIDNSHP=X with lengths of 1 .. 9 digits below 2^28",
    "CIGAR has more than 65535 operations (the CG form is not built)",
    "RNEXT is not *, = or one of the header's references",
    "PNEXT is not a number in 0 .. 2^31 - 1",
    "TLEN is not a number in -2^31 .. 2^31 - 1",
    "QUAL and SEQ differ in length",
    "an attribute is not TAG:TYPE:VALUE with a type of AifZHB",
    "an i attribute is not a number in -2^31 .. 2^32 - 1",
    "an f attribute is not inf, -inf, nan or a decimal of at most 15 significant digits and a power of ten within 22",
    "a B attribute has no subtype of cCsSiIf or a value outside its subtype",
};

// what K-SAM-SIZE leaves for K-SAM-WRITE: the end of each of the eleven fields in the line and the record's first 36 bytes
struct SvLine {
    uint32_t tab[11];
    uint32_t core[9];
};

// ---- the rules one lane applies to its own bytes (the host loop applies the same) -------------------------------------------------------
SV_HD bool sv_digit(uint8_t c) { return (uint8_t)(c - '0') < 10; }

// [-+]?[0-9]{1,10} (the sign where `sign`)
SV_HD bool sv_int(const uint8_t *p, uint32_t b, uint32_t e, bool sign, int64_t &v) {
    bool neg = false;
    if (sign && b < e && (p[b] == '-' || p[b] == '+')) neg = p[b++] == '-';
    if (b >= e || e - b > 10) return false;
    int64_t x = 0;
    for (; b < e; b++) {
        if (!sv_digit(p[b])) return false;
        x = x * 10 + (p[b] - '0');
    }
    v = neg ? -x : x;
    return true;
}

// a float text of the class DESIGN.md 8n names -> the bits of struct.pack('<f', float(text)): the digits are an exact integer below 10^15
// in a double, the power of ten is exact up to 10^22, so the one multiplication or division rounds once, as a correctly rounding
// strtod does; the conversion to float rounds to nearest even in both
SV_HD bool sv_float(const uint8_t *p, uint32_t b, uint32_t e, uint32_t &bits) {
    const uint32_t n = e - b;
    if (n == 3 && p[b] == 'i' && p[b + 1] == 'n' && p[b + 2] == 'f') return bits = 0x7F800000u, true;
    if (n == 4 && p[b] == '-' && p[b + 1] == 'i' && p[b + 2] == 'n' && p[b + 3] == 'f') return bits = 0xFF800000u, true;
    if (n == 3 && p[b] == 'n' && p[b + 1] == 'a' && p[b + 2] == 'n') return bits = 0x7FC00000u, true;
    bool neg = false, dot = false;
    if (b < e && (p[b] == '-' || p[b] == '+')) neg = p[b++] == '-';
    uint64_t m = 0;
    int32_t sig = 0, frac = 0, nd = 0;
    for (; b < e; b++) {
        const uint8_t c = p[b];
        if (sv_digit(c)) {
            nd++;
            if (m || c != '0')
                if (++sig > 15) return false;
            m = m * 10 + (c - '0');
            frac += dot;
        } else if (c == '.' && !dot) {
            dot = true;
        } else {
            break;
        }
    }
    if (!nd) return false;
    int32_t ex = 0;
    if (b < e) {
        if (p[b] != 'e' && p[b] != 'E') return false;
        b++;
        bool eneg = false;
        if (b < e && (p[b] == '-' || p[b] == '+')) eneg = p[b++] == '-';
        if (b >= e || e - b > 4) return false;
        for (; b < e; b++) {
            if (!sv_digit(p[b])) return false;
            ex = ex * 10 + (p[b] - '0');
        }
        if (eneg) ex = -ex;
    }
    const int32_t pw = ex - frac;
    if (pw < -22 || pw > 22) return false;
    double ten = 1.0;  // 10^|pw|: every partial product is a power of ten below 2^77 with at most 22 factors of 5, exact in a double
    for (int32_t k = pw < 0 ? -pw : pw; k > 0; k--) ten *= 10.0;
    double v = (double)m;
    v = pw < 0 ? v / ten : v * ten;
    const float f = (float)(neg ? -v : v);
    __builtin_memcpy(&bits, &f, 4);
    return true;
}

SV_HD uint8_t sv_int_type(int64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return int_type(v);  // smi_auxedit.h: the type K-EDIT gives the value when it rewrites the record
#else
    return v >= -128 && v <= 127 ? 'c' : v >= 0 && v <= 255 ? 'C' : v >= -32768 && v <= 32767 ? 's' : v >= 0 && v <= 65535 ? 'S' : v >= INT32_MIN && v <= INT32_MAX ? 'i' : 'I';
#endif
}
SV_HD uint32_t sv_width(uint8_t t) { return t == 'c' || t == 'C' ? 1u : t == 's' || t == 'S' ? 2u : t == 'i' || t == 'I' || t == 'f' ? 4u : 0u; }
SV_HD bool sv_in_type(uint8_t t, int64_t v) {
    switch (t) {
        case 'c': return v >= -128 && v <= 127;
        case 'C': return v >= 0 && v <= 255;
        case 's': return v >= -32768 && v <= 32767;
        case 'S': return v >= 0 && v <= 65535;
        case 'i': return v >= INT32_MIN && v <= INT32_MAX;
        default: return v >= 0 && v <= (int64_t)UINT32_MAX;
    }
}
SV_HD void sv_put(uint8_t *o, uint64_t v, uint32_t n) {
    for (uint32_t k = 0; k < n; k++) o[k] = (uint8_t)(v >> (8 * k));
}
SV_HD void sv_stop(uint32_t &err, uint32_t why) { err = why < err ? why : err; }

// the attribute p[b .. e) (between two tabs) -> its bytes in the record, written at o (WRITE); 0 and err at a stop
template <bool WRITE>
SV_HD uint32_t sv_attr(const uint8_t *p, uint32_t b, uint32_t e, uint8_t *o, uint32_t &err) {
    if (e - b < 5 || p[b + 2] != ':' || p[b + 4] != ':') return sv_stop(err, kSvAttr), 0u;
    const uint8_t ty = p[b + 3];
    const uint32_t v = b + 5, n = e - v;
    if (WRITE) o[0] = p[b], o[1] = p[b + 1];
    switch (ty) {
        case 'A':
            if (n != 1) return sv_stop(err, kSvAttr), 0u;
            if (WRITE) o[2] = 'A', o[3] = p[v];
            return 4;
        case 'i': {
            int64_t x = 0;
            if (!sv_int(p, v, e, true, x) || x < INT32_MIN || x > (int64_t)UINT32_MAX) return sv_stop(err, kSvAttrInt), 0u;
            const uint8_t t = sv_int_type(x);
            if (WRITE) o[2] = t, sv_put(o + 3, (uint64_t)x, sv_width(t));
            return 3 + sv_width(t);
        }
        case 'f': {
            uint32_t bits = 0;
            if (!sv_float(p, v, e, bits)) return sv_stop(err, kSvAttrFloat), 0u;
            if (WRITE) o[2] = 'f', sv_put(o + 3, bits, 4);
            return 7;
        }
        case 'Z':
        case 'H':
            if (WRITE) {
                o[2] = ty;
                for (uint32_t k = 0; k < n; k++) o[3 + k] = p[v + k];
                o[3 + n] = 0;
            }
            return 4 + n;
        case 'B': {
            const uint8_t st = n ? p[v] : 0;
            const uint32_t es = sv_width(st);
            if (!es) return sv_stop(err, kSvAttrB), 0u;
            uint32_t q = v + 1, cnt = 0;
            while (q < e) {
                if (p[q] != ',') return sv_stop(err, kSvAttrB), 0u;
                uint32_t r = q + 1;
                while (r < e && p[r] != ',') r++;
                uint64_t val = 0;
                if (st == 'f') {
                    uint32_t bits = 0;
                    if (!sv_float(p, q + 1, r, bits)) return sv_stop(err, kSvAttrB), 0u;
                    val = bits;
                } else {
                    int64_t x = 0;
                    if (!sv_int(p, q + 1, r, true, x) || !sv_in_type(st, x)) return sv_stop(err, kSvAttrB), 0u;
                    val = (uint64_t)x;
                }
                if (WRITE) sv_put(o + 8 + cnt * es, val, es);
                cnt++;
                q = r;
            }
            if (WRITE) o[2] = 'B', o[3] = st, sv_put(o + 4, cnt, 4);
            return 8 + cnt * es;
        }
        default: return sv_stop(err, kSvAttr), 0u;
    }
}

// 4-bit code of a base over =ACMGRSVTWYHKDBN, either case; any other byte is N
SV_HD uint32_t sv_base(uint8_t c) {
    if (c == '=') return 0;
    const uint32_t u = (uint32_t)(c & 0xDFu) - 'A';
    if (u > 25) return 15;
    return (uint32_t)((u < 16 ? 0xFFF3FCFFB4FFD2E1ull >> (4 * u) : 0xFFFFFFFAF97F865Full >> (4 * (u - 16))) & 15u);  // A .. P, Q .. Z
}
SV_HD uint32_t sv_cigar_code(uint8_t c) {
    const char *ops = "MIDNSHP=X";
    for (uint32_t k = 0; k < 9; k++)
        if (c == (uint8_t)ops[k]) return k;
    return 9;
}
SV_HD bool sv_on_reference(uint32_t code) { return (0x18Du >> code) & 1u; }  // M D N = X
SV_HD uint32_t sv_reg2bin(int64_t beg, int64_t end) {
    end--;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}
// the 36 fixed bytes: pos and next_pos are the text's values minus 1; bin keeps its low 16 bits
SV_HD void sv_core(uint32_t *core, uint32_t size, int32_t ref, int64_t pos, uint32_t mapq, uint32_t flag, uint32_t l_name, uint32_t n_ops, uint32_t l_seq,
                   int32_t next_ref, int64_t next_pos, int64_t tlen, uint64_t ref_len) {
    const uint32_t bin = pos < 0 ? 4680u : sv_reg2bin(pos, pos + (int64_t)(ref_len ? ref_len : 1)) & 0xFFFFu;
    core[0] = size - 4;
    core[1] = (uint32_t)ref;
    core[2] = (uint32_t)pos;
    core[3] = bin << 16 | mapq << 8 | l_name;
    core[4] = flag << 16 | n_ops;
    core[5] = l_seq;
    core[6] = (uint32_t)next_ref;
    core[7] = (uint32_t)next_pos;
    core[8] = (uint32_t)tlen;
}

// ---- the wavefront's steps --------------------------------------------------------------------------------------------------------------
// the four bytes of the line at `at`, bytes at or behind `end` replaced by fill's; the last one to three bytes in front of `end` come singly
__device__ __forceinline__ uint32_t sv_load4(const uint8_t *__restrict__ p, uint32_t at, uint32_t end, uint32_t fill) {
    uint32_t w = fill;
    if (at + 4 <= end) {
        __builtin_memcpy(&w, p + at, 4);
    } else if (at < end) {
        for (uint32_t k = 0; k < end - at; k++) w = (w & ~(0xFFu << (8 * k))) | (uint32_t)p[at + k] << (8 * k);
    }
    return w;
}
// 0x80 in every byte of w that is a tab
__device__ __forceinline__ uint32_t sv_tabs(uint32_t w) {
    const uint32_t x = w ^ 0x09090909u;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}
// 0x80 in every byte of w that is no digit
__device__ __forceinline__ uint32_t sv_non_digits(uint32_t w) {
    uint32_t m = 0;
    for (int k = 0; k < 4; k++) m |= sv_digit((uint8_t)(w >> (8 * k))) ? 0u : 0x80u << (8 * k);
    return m;
}
// marks (0x80 per byte) in the wavefront's 256 bytes: how many stand in front of this lane's four bytes, and how many there are
struct SvOrd {
    uint32_t before, total;
};
__device__ __forceinline__ SvOrd sv_ord(uint32_t m, int lane) {
    const unsigned long long lt = (1ull << lane) - 1ull;
    SvOrd o = {0, 0};
    for (int k = 0; k < 4; k++) {
        const unsigned long long b = __ballot((m >> (8 * k + 7)) & 1u);
        o.before += __popcll(b & lt);
        o.total += __popcll(b);
    }
    return o;
}
template <class T>
__device__ __forceinline__ T sv_wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) {
        if constexpr (sizeof(T) == 8) v += (T)__shfl_xor((long long)v, o);
        else v += __shfl_xor(v, o);
    }
    return v;
}
__device__ __forceinline__ uint32_t sv_wave_min(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// RNAME / RNEXT p[b .. e): -1 for *, -3 for = (RNEXT), the reference's number, -2 for a name the header does not have
struct SvRefs {
    const uint32_t *slots;  // open addressing over the @SQ names, entry numbers; mask + 1 slots (none where n_ref == 0)
    uint32_t mask;
    const uint8_t *names;      // the names back to back
    const uint32_t *name_off;  // [n_ref + 1]
    int32_t n_ref;
};
__device__ __forceinline__ int32_t sv_ref(const uint8_t *__restrict__ p, uint32_t b, uint32_t e, bool rnext, const SvRefs &R) {
    if (e - b == 1 && p[b] == '*') return -1;
    if (rnext && e - b == 1 && p[b] == '=') return -3;
    if (e == b || !R.n_ref) return -2;
    const Bytes mine = {p + b, e - b};
    const Probed r = probe<false>(const_cast<uint32_t *>(R.slots), R.mask, (uint32_t)fnv1a(mine.p, mine.n) & R.mask, 0u, mine, [&](uint32_t en) {
        return Bytes{R.names + R.name_off[en], R.name_off[en + 1] - R.name_off[en]};
    });
    return r.entry == kEmpty ? -2 : (int32_t)r.entry;
}

// The CIGAR p[b .. e): the lane whose four bytes hold an operation's letter takes that operation (its length: the digits in front of the
// letter, walked back by that lane) -> the number of operations; !WRITE: the rules and the length on the reference; WRITE: the words at o
template <bool WRITE>
__device__ __forceinline__ uint32_t sv_cigar(const uint8_t *__restrict__ p, uint32_t b, uint32_t e, int lane, uint8_t *__restrict__ o, uint64_t &ref_len,
                                             uint32_t &err) {
    ref_len = 0;
    if (e - b == 1 && p[b] == '*') return 0;
    if (e == b) return sv_stop(err, kSvCigar), 0u;
    uint32_t n_ops = 0;
    uint64_t mine = 0;
    for (uint32_t c0 = b; c0 < e; c0 += kSvStep) {
        const uint32_t at = c0 + 4 * lane;
        const uint32_t w = sv_load4(p, at, e, 0x30303030u), m = sv_non_digits(w);
        const SvOrd ord = sv_ord(m, lane);
        uint32_t k = n_ops + ord.before;
        for (int j = 0; m && j < 4; j++) {
            if (!((m >> (8 * j + 7)) & 1u)) continue;
            const uint32_t at_op = at + j, code = sv_cigar_code((uint8_t)(w >> (8 * j)));
            uint32_t q = at_op, nd = 0;
            while (q > b && nd < 10 && sv_digit(p[q - 1])) q--, nd++;
            uint64_t len = 0;
            for (; q < at_op; q++) len = len * 10 + (p[q] - '0');
            if (!WRITE) {
                if (code > 8 || nd < 1 || nd > 9 || len >= (1u << 28)) sv_stop(err, kSvCigar);
                if (code <= 8 && sv_on_reference(code)) mine += len;
            } else if (k < 65535u) {
                st_u32(o + 4 * (size_t)k, (uint32_t)len << 4 | code);
            }
            k++;
        }
        n_ops += ord.total;
    }
    if (!WRITE) {
        if (sv_digit(p[e - 1])) sv_stop(err, kSvCigar);  // digits without an operation behind them
        if (n_ops > 65535u) sv_stop(err, kSvCigarMany);
        ref_len = sv_wave_sum(mine);
    }
    return n_ops;
}

// The attributes of the line: p[from] is the tab behind QUAL (from == L: none).  The lane whose four bytes hold a tab takes the attribute
// behind it -> the bytes all of them take; WRITE: each at its place in text order, by a prefix sum of the sizes over the lanes
template <bool WRITE>
__device__ __forceinline__ uint32_t sv_attrs(const uint8_t *__restrict__ p, uint32_t from, uint32_t L, int lane, uint8_t *__restrict__ o, uint32_t &err) {
    uint32_t total = 0;
    for (uint32_t c0 = from; c0 < L; c0 += kSvStep) {
        const uint32_t at = c0 + 4 * lane, m = sv_tabs(sv_load4(p, at, L, 0u));
        if (!__ballot(m != 0)) continue;
        uint32_t mine = 0, unused = kSvNone;
        for (int j = 0; m && j < 4; j++) {
            if (!((m >> (8 * j + 7)) & 1u)) continue;
            const uint32_t ab = at + j + 1;
            uint32_t ae = ab;
            while (ae < L && p[ae] != '\t') ae++;
            mine += sv_attr<false>(p, ab, ae, nullptr, WRITE ? unused : err);
        }
        if (!WRITE) {
            total += sv_wave_sum(mine);
            continue;
        }
        const uint32_t incl = wave_incl_sum(mine, lane);
        uint32_t to = total + incl - mine;
        for (int j = 0; m && j < 4; j++) {
            if (!((m >> (8 * j + 7)) & 1u)) continue;
            const uint32_t ab = at + j + 1;
            uint32_t ae = ab;
            while (ae < L && p[ae] != '\t') ae++;
            to += sv_attr<true>(p, ab, ae, o + to, unused);
        }
        total += __shfl(incl, 63);
    }
    return total;
}

// SEQ s[0 .. n) -> (n + 1) / 2 bytes at d: a lane takes eight bases to one aligned 32-bit word; the bytes in front of the first aligned
// address and behind the last whole word (fewer than four of either, the last with one base where n is odd) go one per lane
__device__ __forceinline__ void sv_seq(const uint8_t *__restrict__ s, uint32_t n, uint8_t *__restrict__ d, int lane) {
    const uint32_t nb = (n + 1) / 2, full = n / 2;
    const uint32_t want = (uint32_t)(-(intptr_t)d) & 3u, head = want < nb ? want : nb;
    const auto two = [&](uint32_t k) { return (uint8_t)(sv_base(s[2 * k]) << 4 | (2 * k + 1 < n ? sv_base(s[2 * k + 1]) : 0u)); };
    if ((uint32_t)lane < head) d[lane] = two(lane);
    const uint32_t words = full > head ? (full - head) / 4 : 0;
    for (uint32_t w = lane; w < words; w += 64) {
        uint2 v;
        __builtin_memcpy(&v, s + 2 * (size_t)(head + 4 * w), 8);
        uint32_t out = 0;
        for (int k = 0; k < 2; k++) {
            out |= (sv_base((uint8_t)(v.x >> (16 * k))) << 4 | sv_base((uint8_t)(v.x >> (16 * k + 8)))) << (8 * k);
            out |= (sv_base((uint8_t)(v.y >> (16 * k))) << 4 | sv_base((uint8_t)(v.y >> (16 * k + 8)))) << (8 * k + 16);
        }
        *reinterpret_cast<uint32_t *>(__builtin_assume_aligned(d + head + 4 * (size_t)w, 4)) = out;
    }
    const uint32_t done = head + 4 * words;
    if (done + lane < nb) d[done + lane] = two(done + lane);
}

// QUAL s[0 .. n) minus 33 (s == nullptr: 0xFF) -> n bytes at d, four to an aligned word per lane, head and tail one byte per lane
__device__ __forceinline__ void sv_qual(const uint8_t *__restrict__ s, uint32_t n, uint8_t *__restrict__ d, int lane) {
    const uint32_t want = (uint32_t)(-(intptr_t)d) & 3u, head = want < n ? want : n;
    if ((uint32_t)lane < head) d[lane] = s ? (uint8_t)(s[lane] - 33) : 0xFFu;
    const uint32_t words = (n - head) / 4;
    for (uint32_t w = lane; w < words; w += 64) {
        uint32_t x = 0xFFFFFFFFu;
        if (s) {
            __builtin_memcpy(&x, s + head + 4 * (size_t)w, 4);
            x = ((x | 0x80808080u) - 0x21212121u) ^ (~x & 0x80808080u);  // every byte minus 33, no borrow between bytes
        }
        *reinterpret_cast<uint32_t *>(__builtin_assume_aligned(d + head + 4 * (size_t)w, 4)) = x;
    }
    const uint32_t done = head + 4 * words;
    if (done + lane < n) d[done + lane] = s ? (uint8_t)(s[done + lane] - 33) : 0xFFu;
}

// K-SAM-SIZE: line i of the segment is text[line_start[i] .. line_start[i + 1] - 1)
__global__ __launch_bounds__(kSvBlock) void k_sam_size(const uint8_t *__restrict__ text, const uint64_t *__restrict__ line_start, uint32_t n_lines, SvRefs R,
                                                       SvLine *__restrict__ lines, uint64_t *__restrict__ size, unsigned long long *__restrict__ stop) {
    __shared__ uint32_t s_tab[kSvWaves][12];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * kSvWaves + wv;
    if (i >= n_lines) return;
    const uint64_t b0 = line_start[i];
    const uint32_t L = (uint32_t)(line_start[i + 1] - 1 - b0);
    const uint8_t *__restrict__ p = text + b0;
    uint32_t *T = s_tab[wv];
    // the first eleven tabs; a field that the line's end closes ends at L
    if (lane < 11) T[lane] = L;
    wave_sync();
    uint32_t nt = 0;
    for (uint32_t c0 = 0; c0 < L && nt < 11; c0 += kSvStep) {
        const uint32_t at = c0 + 4 * lane, m = sv_tabs(sv_load4(p, at, L, 0u));
        const SvOrd ord = sv_ord(m, lane);
        uint32_t k = nt + ord.before;
        for (int j = 0; m && j < 4; j++)
            if ((m >> (8 * j + 7)) & 1u) {
                if (k < 11) T[k] = at + j;
                k++;
            }
        nt += ord.total;
    }
    wave_sync();
    uint32_t err = kSvNone;
    if (L && p[0] == '@') sv_stop(err, kSvLate);
    if (nt < 10) sv_stop(err, kSvFields);
    if (err != kSvNone) {  // (the same in every lane)
        if (lane == 0) {
            atomicMin(stop, (unsigned long long)i << 6 | err);
            size[i] = 0;
        }
        return;
    }
    const uint32_t t0 = T[0], t1 = T[1], t2 = T[2], t3 = T[3], t4 = T[4], t5 = T[5], t6 = T[6], t7 = T[7], t8 = T[8], t9 = T[9], t10 = T[10];
    // the numbers and the two reference names: a lane each
    int64_t val = 0;
    switch (lane) {
        case 0:
            if (t0 < 1 || t0 > 254) sv_stop(err, kSvName);
            break;
        case 1:
            if (!sv_int(p, t0 + 1, t1, false, val) || val > 65535) sv_stop(err, kSvFlag);
            break;
        case 2:
            val = sv_ref(p, t1 + 1, t2, false, R);
            if (val == -2) sv_stop(err, kSvRname);
            break;
        case 3:
            if (!sv_int(p, t2 + 1, t3, false, val) || val > INT32_MAX) sv_stop(err, kSvPos);
            val--;
            break;
        case 4:
            if (!sv_int(p, t3 + 1, t4, false, val) || val > 255) sv_stop(err, kSvMapq);
            break;
        case 5:
            val = sv_ref(p, t5 + 1, t6, true, R);
            if (val == -2) sv_stop(err, kSvRnext);
            break;
        case 6:
            if (!sv_int(p, t6 + 1, t7, false, val) || val > INT32_MAX) sv_stop(err, kSvPnext);
            val--;
            break;
        case 7:
            if (!sv_int(p, t7 + 1, t8, true, val) || val < INT32_MIN || val > INT32_MAX) sv_stop(err, kSvTlen);
            break;
        default: break;
    }
    const int32_t v32 = (int32_t)val;
    const uint32_t flag = (uint32_t)__shfl(v32, 1), mapq = (uint32_t)__shfl(v32, 4);
    const int32_t ref = __shfl(v32, 2), pos = __shfl(v32, 3), next_pos = __shfl(v32, 6), tlen = __shfl(v32, 7);
    int32_t next_ref = __shfl(v32, 5);
    if (next_ref == -3) next_ref = ref;
    uint64_t ref_len = 0;
    const uint32_t n_ops = sv_cigar<false>(p, t4 + 1, t5, lane, nullptr, ref_len, err);
    const uint32_t l_seq = t9 - t8 - 1 == 1 && p[t8 + 1] == '*' ? 0u : t9 - t8 - 1;
    const bool no_qual = t10 - t9 - 1 == 1 && p[t9 + 1] == '*';
    if (!no_qual && t10 - t9 - 1 != l_seq) sv_stop(err, kSvQualLen);
    const uint32_t aux = sv_attrs<false>(p, t10, L, lane, nullptr, err);
    err = sv_wave_min(err);
    const uint64_t bytes = 36ull + (t0 + 1) + 4ull * n_ops + (l_seq + 1) / 2 + (uint64_t)l_seq + aux;
    if (err == kSvNone && bytes > UINT32_MAX) err = kSvFields;  // (cannot happen: a segment is below 2^31 bytes and a record at most twice its line)
    if (err != kSvNone) {
        if (lane == 0) {
            atomicMin(stop, (unsigned long long)i << 6 | err);
            size[i] = 0;
        }
        return;
    }
    if (lane < 11) lines[i].tab[lane] = T[lane];
    if (lane == 0) {
        uint32_t core[9];
        sv_core(core, (uint32_t)bytes, ref, pos, mapq, flag, t0 + 1, n_ops, l_seq, next_ref, next_pos, tlen, ref_len);
        for (int k = 0; k < 9; k++) lines[i].core[k] = core[k];
        size[i] = bytes;
    }
}

// K-SAM-WRITE: the record of line i at out + off[i]
__global__ __launch_bounds__(kSvBlock) void k_sam_write(const uint8_t *__restrict__ text, const uint64_t *__restrict__ line_start, uint32_t n_lines,
                                                        const SvLine *__restrict__ lines, const uint64_t *__restrict__ off, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * kSvWaves + (threadIdx.x >> 6);
    if (i >= n_lines) return;
    const uint64_t b0 = line_start[i];
    const uint32_t L = (uint32_t)(line_start[i + 1] - 1 - b0);
    const uint8_t *__restrict__ p = text + b0;
    const SvLine *__restrict__ ln = lines + i;
    uint8_t *__restrict__ rec = out + off[i];
    const uint32_t t0 = ln->tab[0], t4 = ln->tab[4], t5 = ln->tab[5], t8 = ln->tab[8], t9 = ln->tab[9], t10 = ln->tab[10];
    const uint32_t l_name = t0 + 1, n_ops = ln->core[4] & 0xFFFFu, l_seq = ln->core[5];
    if (lane < 36) rec[lane] = (uint8_t)(ln->core[lane >> 2] >> (8 * (lane & 3)));
    wave_copy(rec + 36, p, t0, lane);
    if (lane == 0) rec[36 + t0] = 0;
    uint32_t unused = kSvNone;
    uint64_t ref_len;
    uint8_t *at = rec + 36 + l_name;
    sv_cigar<true>(p, t4 + 1, t5, lane, at, ref_len, unused);
    at += 4 * (size_t)n_ops;
    sv_seq(p + t8 + 1, l_seq, at, lane);
    at += (l_seq + 1) / 2;
    const bool no_qual = t10 - t9 - 1 == 1 && p[t9 + 1] == '*';
    sv_qual(no_qual ? nullptr : p + t9 + 1, l_seq, at, lane);
    at += l_seq;
    sv_attrs<true>(p, t10, L, lane, at, unused);
}

template <class T>
int sv_grow(T **p, size_t &cap, size_t want) {
    if (want <= cap && *p) return SMI_OK;
    const size_t n = std::max<size_t>(want + want / 4, 1024);
    if (*p) SMI_HIP(hipFree(*p));
    *p = nullptr;
    cap = 0;
    if (hipMalloc((void **)p, n * sizeof(T)) != hipSuccess) {
        *p = nullptr;
        set_error("SamView: device allocation of " + std::to_string(n * sizeof(T)) + " bytes failed");
        return SMI_ERR_HIP;
    }
    cap = n;
    return SMI_OK;
}

inline uint64_t sv_hash(const std::string &s) {
    uint64_t h = kFnvBasis;
    for (unsigned char c : s) h = fnv1a_add(h, c);
    return h;
}

// the same conversion of one line on the host (smi_samview_host_loop): the record appended to out, or false at a stop
bool sv_host_line(const uint8_t *p, uint32_t L, const std::unordered_map<std::string, int32_t> &refs, std::vector<uint8_t> &out) {
    uint32_t t[11];
    uint32_t nt = 0;
    for (uint32_t k = 0; k < L && nt < 11; k++)
        if (p[k] == '\t') t[nt++] = k;
    if (nt < 10 || p[0] == '@') return false;
    if (nt == 10) t[10] = L;
    uint32_t err = kSvNone;
    int64_t flag = 0, pos = 0, mapq = 0, pnext = 0, tlen = 0;
    if (t[0] < 1 || t[0] > 254) return false;
    if (!sv_int(p, t[0] + 1, t[1], false, flag) || flag > 65535) return false;
    if (!sv_int(p, t[2] + 1, t[3], false, pos) || pos > INT32_MAX) return false;
    if (!sv_int(p, t[3] + 1, t[4], false, mapq) || mapq > 255) return false;
    if (!sv_int(p, t[6] + 1, t[7], false, pnext) || pnext > INT32_MAX) return false;
    if (!sv_int(p, t[7] + 1, t[8], true, tlen) || tlen < INT32_MIN || tlen > INT32_MAX) return false;
    const auto ref_of = [&](uint32_t b, uint32_t e, bool rnext, int32_t same) -> int32_t {
        if (e - b == 1 && p[b] == '*') return -1;
        if (rnext && e - b == 1 && p[b] == '=') return same;
        const auto it = refs.find(std::string((const char *)p + b, e - b));
        return it == refs.end() ? -2 : it->second;
    };
    const int32_t ref = ref_of(t[1] + 1, t[2], false, 0), next_ref = ref_of(t[5] + 1, t[6], true, ref);
    if (ref == -2 || next_ref == -2) return false;
    std::vector<uint32_t> ops;
    uint64_t ref_len = 0;
    if (!(t[5] - t[4] - 1 == 1 && p[t[4] + 1] == '*')) {
        uint32_t q = t[4] + 1;
        if (q == t[5]) return false;
        while (q < t[5]) {
            uint64_t len = 0;
            uint32_t nd = 0;
            while (q < t[5] && sv_digit(p[q]) && nd < 10) len = len * 10 + (p[q++] - '0'), nd++;
            const uint32_t code = q < t[5] ? sv_cigar_code(p[q]) : 9;
            if (code > 8 || nd < 1 || nd > 9 || len >= (1u << 28)) return false;
            if (sv_on_reference(code)) ref_len += len;
            ops.push_back((uint32_t)len << 4 | code);
            q++;
        }
        if (ops.size() > 65535) return false;
    }
    const uint32_t sb = t[8] + 1, qb = t[9] + 1;
    const uint32_t l_seq = t[9] - sb == 1 && p[sb] == '*' ? 0u : t[9] - sb;
    const bool no_qual = t[10] - qb == 1 && p[qb] == '*';
    if (!no_qual && t[10] - qb != l_seq) return false;
    const size_t at0 = out.size();
    out.resize(at0 + 36 + t[0] + 1 + 4 * ops.size() + (l_seq + 1) / 2 + l_seq);
    uint8_t *o = out.data() + at0 + 36;
    std::memcpy(o, p, t[0]);
    o[t[0]] = 0;
    o += t[0] + 1;
    if (!ops.empty()) std::memcpy(o, ops.data(), 4 * ops.size());
    o += 4 * ops.size();
    for (uint32_t k = 0; k < (l_seq + 1) / 2; k++) o[k] = (uint8_t)(sv_base(p[sb + 2 * k]) << 4 | (2 * k + 1 < l_seq ? sv_base(p[sb + 2 * k + 1]) : 0u));
    o += (l_seq + 1) / 2;
    for (uint32_t k = 0; k < l_seq; k++) o[k] = no_qual ? 0xFFu : (uint8_t)(p[qb + k] - 33);
    uint32_t b = t[10];
    while (b < L) {  // p[b] is the tab in front of an attribute
        uint32_t e = b + 1;
        while (e < L && p[e] != '\t') e++;
        const uint32_t n = sv_attr<false>(p, b + 1, e, nullptr, err);
        if (err != kSvNone) return false;
        const size_t at = out.size();
        out.resize(at + n);
        sv_attr<true>(p, b + 1, e, out.data() + at, err);
        b = e;
    }
    uint32_t core[9];
    sv_core(core, (uint32_t)(out.size() - at0), ref, pos - 1, (uint32_t)mapq, (uint32_t)flag, t[0] + 1, (uint32_t)ops.size(), l_seq, next_ref, pnext - 1, tlen, ref_len);
    std::memcpy(out.data() + at0, core, 36);
    return true;
}

}  // namespace
}  // namespace smi

using namespace smi;

struct smi_samview {
    smi_ctx *ctx = nullptr;
    std::string header;  // the BAM header: magic, l_text, text, n_ref, the references
    std::vector<std::string> ref_names;
    std::unordered_map<std::string, int32_t> ref_of;  // the first @SQ line of a name
    // the @SQ names on the device
    uint32_t *d_slots = nullptr, *d_name_off = nullptr;
    uint8_t *d_names = nullptr;
    uint32_t mask = 0;
    // one segment (grow-only)
    uint8_t *d_text = nullptr, *d_out = nullptr;
    uint64_t *d_line = nullptr, *d_off = nullptr;
    SvLine *d_lines = nullptr;
    size_t text_cap = 0, out_cap = 0, line_cap = 0, off_cap = 0, lines_cap = 0;
    unsigned long long *d_stop = nullptr;
    Scratch cub{"SamView"};
    size_t n_text = 0, n_lines = 0, n_out = 0;  // of the segment taken last
    bool sized = false, written = false, failed = false;
    int64_t line_base = 0;  // lines in front of the segment: the header's, then every segment's
    Events ev;
    int64_t counts[SMI_SAMVIEW_N_COUNT] = {};
    float ms[SMI_SAMVIEW_N_STAGE] = {};
    int64_t error_line = 0;
    std::string error_reason;
};

namespace {

void sv_release(smi_samview *h) {
    void *bufs[] = {h->d_slots, h->d_name_off, h->d_names, h->d_text, h->d_out, h->d_line, h->d_off, h->d_lines, h->d_stop};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    delete h;
}

int sv_stop_at(smi_samview *h, int64_t line, const std::string &why) {
    h->failed = true;
    h->error_line = line;
    h->error_reason = why;
    set_error("line " + std::to_string(line) + ": " + why);
    return 2;
}

// the header text -> the BAM header and the references; 2 at an @SQ line without SN or LN
int sv_header(smi_samview *h, const uint8_t *text, size_t n) {
    std::string refs;
    int64_t line = 0;
    for (size_t b = 0; b < n;) {
        size_t e = b;
        while (e < n && text[e] != '\n') e++;
        line++;
        const std::string_view ln((const char *)text + b, e - b);
        if (ln.substr(0, 4) == "@SQ\t" || ln == "@SQ") {
            std::string name;
            int64_t len = -1;
            bool has_name = false;
            for (const auto f : lr::jsplit(ln, '\t')) {
                if (f.substr(0, 3) == "SN:" && !has_name) name = std::string(f.substr(3)), has_name = true;
                if (f.substr(0, 3) == "LN:" && len < 0) {
                    int64_t v = 0;
                    if (sv_int((const uint8_t *)f.data(), 3, (uint32_t)f.size(), false, v) && v <= INT32_MAX) len = v;
                }
            }
            if (!has_name || name.empty() || len < 0) return sv_stop_at(h, line, "an @SQ line without SN or an LN in 0 .. 2^31 - 1");
            const uint32_t l_name = (uint32_t)name.size() + 1, l_ref = (uint32_t)len;
            refs.append((const char *)&l_name, 4).append(name).push_back('\0');
            refs.append((const char *)&l_ref, 4);
            h->ref_of.emplace(name, (int32_t)h->ref_names.size());
            h->ref_names.push_back(name);
        }
        b = e + 1;
    }
    h->line_base = line;
    const uint32_t l_text = (uint32_t)n, n_ref = (uint32_t)h->ref_names.size();
    h->header.assign("BAM\1", 4).append((const char *)&l_text, 4).append((const char *)text, n).append((const char *)&n_ref, 4).append(refs);
    return SMI_OK;
}

int sv_upload_refs(smi_samview *h) {
    const size_t n = h->ref_names.size();
    if (!n) return SMI_OK;
    size_t slots = 2;
    while (slots < 2 * n) slots <<= 1;
    std::vector<uint32_t> tab(slots, kEmpty), off(n + 1, 0);
    std::string names;
    for (size_t k = 0; k < n; k++) {
        off[k] = (uint32_t)names.size();
        names += h->ref_names[k];
    }
    off[n] = (uint32_t)names.size();
    for (size_t k = 0; k < n; k++) {
        if (h->ref_of[h->ref_names[k]] != (int32_t)k) continue;  // a later @SQ line of the same name is never found
        size_t s = sv_hash(h->ref_names[k]) & (slots - 1);
        while (tab[s] != kEmpty) s = (s + 1) & (slots - 1);
        tab[s] = (uint32_t)k;
    }
    h->mask = (uint32_t)(slots - 1);
    SMI_HIP(hipMalloc((void **)&h->d_slots, slots * 4));
    SMI_HIP(hipMalloc((void **)&h->d_name_off, (n + 1) * 4));
    SMI_HIP(hipMalloc((void **)&h->d_names, std::max<size_t>(names.size(), 1)));
    SMI_HIP(hipMemcpy(h->d_slots, tab.data(), slots * 4, hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(h->d_name_off, off.data(), (n + 1) * 4, hipMemcpyHostToDevice));
    SMI_HIP(hipMemcpy(h->d_names, names.data(), names.size(), hipMemcpyHostToDevice));
    return SMI_OK;
}

inline unsigned sv_grid(size_t n_lines) { return (unsigned)std::max<size_t>(1, (n_lines + kSvWaves - 1) / kSvWaves); }

int sv_write(smi_samview *h, hipStream_t s) {
    hipLaunchKernelGGL(k_sam_write, dim3(sv_grid(h->n_lines)), dim3(kSvBlock), 0, s, (const uint8_t *)h->d_text, (const uint64_t *)h->d_line, (uint32_t)h->n_lines,
                       (const SvLine *)h->d_lines, (const uint64_t *)h->d_off, h->d_out);
    SMI_HIP(hipGetLastError());
    return SMI_OK;
}

}  // namespace

extern "C" int smi_samview_create(smi_ctx *ctx, const uint8_t *header_text, size_t n_text, smi_samview **out) {
    if (!ctx || !out || (n_text && !header_text) || n_text > (size_t)INT32_MAX) {
        set_error("smi_samview_create: bad argument");
        return SMI_ERR_INVALID;
    }
    *out = nullptr;
    SMI_HIP(hipSetDevice(ctx->device));
    smi_samview *h = new smi_samview();
    h->ctx = ctx;
    *out = h;  // a stop in the header leaves the handle, which names the line
    if (int rc = sv_header(h, header_text, n_text)) return rc;
    int rc = sv_upload_refs(h);
    if (!rc && hipMalloc((void **)&h->d_stop, sizeof(unsigned long long)) != hipSuccess) rc = hip_fail(hipErrorOutOfMemory, "smi_samview_create");
    if (rc) {
        sv_release(h);
        *out = nullptr;
        return rc;
    }
    h->counts[SMI_SAMVIEW_REFERENCES] = (int64_t)h->ref_names.size();
    return SMI_OK;
}

extern "C" int smi_samview_free(smi_samview *h) {
    if (h) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        sv_release(h);
    }
    return SMI_OK;
}

extern "C" int smi_samview_header(const smi_samview *h, uint8_t *out, size_t cap, size_t *n_out) {
    if (!h || !n_out) {
        set_error("smi_samview_header: null argument");
        return SMI_ERR_INVALID;
    }
    return handle::get_text(h->header, out, cap, n_out);
}

extern "C" int smi_samview_counts(const smi_samview *h, int64_t *counts) {
    if (!h || !counts) {
        set_error("smi_samview_counts: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(counts, h->counts, sizeof h->counts);
    return SMI_OK;
}

extern "C" int smi_samview_stage_ms(const smi_samview *h, float *ms) {
    if (!h || !ms) {
        set_error("smi_samview_stage_ms: null argument");
        return SMI_ERR_INVALID;
    }
    std::memcpy(ms, h->ms, sizeof h->ms);
    return SMI_OK;
}

extern "C" int smi_samview_error_line(const smi_samview *h, int64_t *line, char *reason, size_t cap) {
    if (!h || !line || (cap && !reason)) {
        set_error("smi_samview_error_line: null argument");
        return SMI_ERR_INVALID;
    }
    return handle::error_read(h->error_reason, h->error_line, reason, cap, line);
}

extern "C" int smi_samview_add_segment(smi_samview *h, const uint8_t *text, size_t n_bytes, size_t *n_bgzf, size_t *n_records_bytes) {
    if (!h || !n_bgzf || !n_records_bytes || (n_bytes && !text)) {
        set_error("smi_samview_add_segment: null argument");
        return SMI_ERR_INVALID;
    }
    *n_bgzf = *n_records_bytes = 0;
    if (h->failed) {
        set_error("smi_samview_add_segment: an earlier call failed");
        return SMI_ERR_STATE;
    }
    if (n_bytes >= kSvMaxSegment) {
        set_error("SamView: a segment of " + std::to_string(n_bytes) + " bytes; at most 2^31 - 1 are taken at once: pass smaller segments");
        return SMI_ERR_INVALID;
    }
    h->sized = h->written = false;
    h->n_text = h->n_lines = h->n_out = 0;
    std::memset(h->ms, 0, sizeof h->ms);
    if (!n_bytes) {
        h->sized = true;
        return smi_bgzf_deflate_device(h->ctx, h->d_out, 0, nullptr, 0, n_bgzf);
    }
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    if (int rc = sv_grow(&h->d_text, h->text_cap, n_bytes + 16)) return rc;
    h->failed = true;  // until the segment is through
    SMI_HIP(hipMemcpyAsync(h->d_text, text, n_bytes, hipMemcpyHostToDevice, s));
    if (int rc = h->ev.begin(s)) return rc;
    size_t swept = 0;
    if (int rc = launch_fastq_sweep(h->ctx, h->d_text, n_bytes, &swept, s)) return rc;
    // bytes behind the last LF are a line: it ends as if an LF stood behind the text
    const bool open_end = text[n_bytes - 1] != '\n';
    const size_t n_nl = swept - (open_end ? 1 : 0), n = swept;
    if (n >= (size_t)INT32_MAX - 1) {  // hipcub counts in int
        set_error("SamView: " + std::to_string(n) + " lines in one segment; at most 2^31 - 3 are taken at once: pass smaller segments");
        return SMI_ERR_INVALID;
    }
    if (int rc = sv_grow(&h->d_line, h->line_cap, n + 1)) return rc;
    if (int rc = sv_grow(&h->d_off, h->off_cap, n + 1)) return rc;
    if (int rc = sv_grow(&h->d_lines, h->lines_cap, n)) return rc;
    if (int rc = launch_fastq_line_starts(h->ctx, h->d_text, n_bytes, h->d_line, n_nl + 1, s)) return rc;
    const uint64_t behind = (uint64_t)n_bytes + 1;
    if (open_end) SMI_HIP(hipMemcpyAsync(h->d_line + n, &behind, 8, hipMemcpyHostToDevice, s));
    if (int rc = h->ev.end(s, &h->ms[SMI_SAMVIEW_MS_INDEX])) return rc;
    const auto offsets = [&](void *p, size_t &t) { return hipcub::DeviceScan::ExclusiveSum(p, t, h->d_off, h->d_off, (int)(n + 1), s); };
    if (int rc = reserve(h->cub, offsets)) return rc;
    SMI_HIP(hipMemsetAsync(h->d_stop, 0xff, sizeof(unsigned long long), s));
    SMI_HIP(hipMemsetAsync(h->d_off + n, 0, 8, s));
    if (int rc = h->ev.begin(s)) return rc;
    const SvRefs R = {h->d_slots, h->mask, h->d_names, h->d_name_off, (int32_t)h->ref_names.size()};
    hipLaunchKernelGGL(k_sam_size, dim3(sv_grid(n)), dim3(kSvBlock), 0, s, (const uint8_t *)h->d_text, (const uint64_t *)h->d_line, (uint32_t)n, R, h->d_lines,
                       h->d_off, h->d_stop);
    SMI_HIP(hipGetLastError());
    if (int rc = h->ev.end(s, &h->ms[SMI_SAMVIEW_MS_SIZE])) return rc;
    if (int rc = h->ev.begin(s)) return rc;
    if (int rc = run_reserved(h->cub, offsets)) return rc;
    if (int rc = h->ev.end(s, &h->ms[SMI_SAMVIEW_MS_SCAN])) return rc;
    unsigned long long stop = kNoStop;
    uint64_t total = 0;
    SMI_HIP(hipMemcpyAsync(&stop, h->d_stop, sizeof stop, hipMemcpyDeviceToHost, s));
    SMI_HIP(hipMemcpyAsync(&total, h->d_off + n, 8, hipMemcpyDeviceToHost, s));
    SMI_HIP(hipStreamSynchronize(s));
    if (stop != kNoStop) {
        const uint32_t why = (uint32_t)(stop & 63u);
        return sv_stop_at(h, h->line_base + (int64_t)(stop >> 6) + 1, kSvReason[why < sizeof kSvReason / sizeof *kSvReason ? why : 0]);
    }
    if (int rc = sv_grow(&h->d_out, h->out_cap, (size_t)total + 16)) return rc;
    h->n_text = n_bytes;
    h->n_lines = n;
    h->n_out = (size_t)total;
    h->sized = true;
    h->failed = false;
    *n_records_bytes = (size_t)total;
    return smi_bgzf_deflate_device(h->ctx, h->d_out, (size_t)total, nullptr, 0, n_bgzf);
}

extern "C" int smi_samview_convert(smi_samview *h, uint8_t *out_bgzf, size_t cap, size_t *n_out, uint8_t *out_records, size_t cap_records) {
    if (!h || !n_out || !out_bgzf) {
        set_error("smi_samview_convert: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed || !h->sized) {
        set_error(h->failed ? "smi_samview_convert: an earlier call failed" : "smi_samview_convert: smi_samview_add_segment comes first");
        return SMI_ERR_STATE;
    }
    size_t bound = 0;
    if (int rc = smi_bgzf_deflate_device(h->ctx, h->d_out, h->n_out, nullptr, 0, &bound)) return rc;
    *n_out = bound;
    if (cap < bound || (out_records && cap_records < h->n_out)) return 1;
    SMI_HIP(hipSetDevice(h->ctx->device));
    hipStream_t s = h->ctx->stream;
    h->ms[SMI_SAMVIEW_MS_WRITE] = h->ms[SMI_SAMVIEW_MS_DEFLATE] = 0.f;
    if (h->n_lines) {
        if (int rc = h->ev.begin(s)) return rc;
        if (int rc = sv_write(h, s)) return rc;
        if (int rc = h->ev.end(s, &h->ms[SMI_SAMVIEW_MS_WRITE])) return rc;
    }
    if (int rc = h->ev.begin(s)) return rc;
    size_t z = 0;
    if (int rc = smi_bgzf_deflate_device(h->ctx, h->d_out, h->n_out, out_bgzf, cap, &z)) return rc;
    if (int rc = h->ev.end(s, &h->ms[SMI_SAMVIEW_MS_DEFLATE])) return rc;
    if (z < 28) {  // (cannot happen: the deflater closes its stream with the end-of-file block)
        set_error("smi_samview_convert: the deflater wrote no end-of-file block");
        return SMI_ERR_STATE;
    }
    *n_out = z - 28;  // the caller ends the file
    if (out_records && h->n_out) SMI_HIP(hipMemcpy(out_records, h->d_out, h->n_out, hipMemcpyDeviceToHost));
    if (!h->written) {
        h->counts[SMI_SAMVIEW_RECORDS] += (int64_t)h->n_lines;
        h->counts[SMI_SAMVIEW_SEGMENTS] += h->n_lines ? 1 : 0;
        h->counts[SMI_SAMVIEW_TEXT_BYTES] += (int64_t)h->n_text;
        h->counts[SMI_SAMVIEW_RECORD_BYTES] += (int64_t)h->n_out;
        h->line_base += (int64_t)h->n_lines;
    }
    h->written = true;
    return SMI_OK;
}

extern "C" int smi_samview_host_loop(smi_samview *h, double *seconds, int64_t *mismatches) {
    if (!h || !seconds || !mismatches) {
        set_error("smi_samview_host_loop: null argument");
        return SMI_ERR_INVALID;
    }
    if (h->failed || !h->written) {
        set_error(h->failed ? "smi_samview_host_loop: an earlier call failed" : "smi_samview_host_loop: smi_samview_convert comes first");
        return SMI_ERR_STATE;
    }
    *seconds = 0.0;
    *mismatches = 0;
    const size_t n = h->n_lines;
    if (!n) return SMI_OK;
    SMI_HIP(hipSetDevice(h->ctx->device));
    // what the device holds comes to the host (not timed): the text, the line table, the records and their offsets
    std::vector<uint8_t> text(h->n_text), dev(h->n_out);
    std::vector<uint64_t> line(n + 1), off(n + 1);
    SMI_HIP(hipMemcpy(text.data(), h->d_text, h->n_text, hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(line.data(), h->d_line, (n + 1) * 8, hipMemcpyDeviceToHost));
    SMI_HIP(hipMemcpy(off.data(), h->d_off, (n + 1) * 8, hipMemcpyDeviceToHost));
    if (h->n_out) SMI_HIP(hipMemcpy(dev.data(), h->d_out, h->n_out, hipMemcpyDeviceToHost));
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> host;
    host.reserve(h->n_out);
    std::vector<uint64_t> at(n + 1);
    std::vector<uint8_t> ok(n);
    for (size_t i = 0; i < n; i++) {
        at[i] = host.size();
        ok[i] = sv_host_line(text.data() + line[i], (uint32_t)(line[i + 1] - 1 - line[i]), h->ref_of, host);
    }
    at[n] = host.size();
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    int64_t bad = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t len = at[i + 1] - at[i];
        if (!ok[i] || off[i + 1] - off[i] != len || off[i] + len > dev.size() || std::memcmp(dev.data() + off[i], host.data() + at[i], len)) bad++;
    }
    *mismatches = bad;
    return SMI_OK;
}
