// smi_longread.h -- the attribute helpers of the LongreadRecord.fromSAMRecord parsers (ComputeConsensus in smi_consensus.hip,
// IsoformMatrix in smi_isoform.hip, SNPMatrix in smi_snp.hip), its CIGAR walk and the Java text rules they share
// (FusionDetector in smi_fusion.hip reads them too): host only.
#pragma once
#include <hip/hip_runtime.h>

#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "sicelore_mi.h"

namespace smi {
namespace lr {

struct Aux {
    const uint8_t *p = nullptr;  // the field (tag, type, value)
    size_t n = 0;
};

// bytes of the attribute at p (tag, type, value) -> 0, or -1 when it is malformed or runs past end
inline int aux_size(const uint8_t *p, const uint8_t *end, size_t *n) {
    if (end - p < 3) return -1;
    const uint8_t t = p[2];
    switch (t) {
        case 'A': case 'c': case 'C': *n = 4; break;
        case 's': case 'S': *n = 5; break;
        case 'i': case 'I': case 'f': *n = 7; break;
        case 'Z': case 'H': {
            const uint8_t *z = (const uint8_t *)std::memchr(p + 3, 0, end - p - 3);
            if (!z) return -1;
            *n = (size_t)(z - p) + 1;
            break;
        }
        case 'B': {
            if (end - p < 8) return -1;
            size_t w;
            switch (p[3]) {
                case 'c': case 'C': w = 1; break;
                case 's': case 'S': w = 2; break;
                case 'i': case 'I': case 'f': w = 4; break;
                default: return -1;
            }
            uint32_t cnt;
            std::memcpy(&cnt, p + 4, 4);
            *n = 8 + w * cnt;
            break;
        }
        default: return -1;
    }
    return p + *n <= end ? 0 : -1;
}

// (Integer) getAttribute: htsjdk boxes c C s S i, and I up to 2^31 - 1, as Integer -> false for any other type
inline bool aux_integer(const Aux &a, int64_t &v) {
    const uint8_t *q = a.p + 3;
    switch (a.p[2]) {
        case 'c': v = (int8_t)q[0]; return true;
        case 'C': v = q[0]; return true;
        case 's': { int16_t x; std::memcpy(&x, q, 2); v = x; return true; }
        case 'S': { uint16_t x; std::memcpy(&x, q, 2); v = x; return true; }
        case 'i': { int32_t x; std::memcpy(&x, q, 4); v = x; return true; }
        case 'I': { uint32_t x; std::memcpy(&x, q, 4); v = x; return x <= 0x7fffffffu; }
    }
    return false;
}

inline bool float_less(float a, float b) {  // Float.compare(a, b) < 0
    if (a < b) return true;
    if (a > b) return false;
    auto bits = [](float x) {
        int32_t i;
        if (x != x) return (int32_t)0x7fc00000;
        std::memcpy(&i, &x, 4);
        return i;
    };
    return bits(a) < bits(b);
}

inline uint16_t tag16(const char *t) { return (uint16_t)((uint8_t)t[0] | (uint8_t)t[1] << 8); }

// LongreadRecord L108-112: the first or the last CIGAR operation is S or H and longer than MAXCLIP
inline bool chimeric(uint32_t first, uint32_t last, int32_t max_clip) {
    auto clip = [&](uint32_t c) { return ((c & 15) == 4 || (c & 15) == 5) && (int64_t)(c >> 4) > (int64_t)max_clip; };
    return clip(first) || clip(last);
}

inline std::string drop_minus1(std::string_view v) {  // String.replace("-1", ""): every occurrence, left to right
    std::string s(v);
    for (size_t k = s.find("-1"); k != std::string::npos; k = s.find("-1", k)) s.erase(k, 2);
    return s;
}

// Java's String.split(regex) for a one-character separator: trailing empty strings removed
inline std::vector<std::string_view> jsplit(std::string_view s, char sep) {
    std::vector<std::string_view> out;
    size_t b = 0;
    for (size_t i = 0; i <= s.size(); i++)
        if (i == s.size() || s[i] == sep) {
            out.push_back(s.substr(b, i - b));
            b = i + 1;
        }
    while (!out.empty() && out.back().empty()) out.pop_back();
    if (s.empty()) out.assign(1, std::string_view());  // "".split(x) = [""]
    return out;
}

// Integer.valueOf
inline bool jint(std::string_view s, int32_t &v) {
    if (s.empty()) return false;
    size_t i = 0;
    bool neg = false;
    if (s[0] == '-' || s[0] == '+') {
        neg = s[0] == '-';
        i = 1;
        if (s.size() == 1) return false;
    }
    int64_t x = 0;
    for (; i < s.size(); i++) {
        if (s[i] < '0' || s[i] > '9') return false;
        x = x * 10 + (s[i] - '0');
        if (x > 2147483648ll) return false;
    }
    if (neg) x = -x;
    if (x > 2147483647ll || x < -2147483648ll) return false;
    v = (int32_t)x;
    return true;
}

// Float.toString: the shortest decimal that reads back as the float; d.ddd in [1e-3, 1e7), else d.dddE<exp>
inline std::string java_float(float x) {
    if (std::isnan(x)) return "NaN";
    if (std::isinf(x)) return x > 0 ? "Infinity" : "-Infinity";
    if (x == 0) return std::signbit(x) ? "-0.0" : "0.0";
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof(buf), x, std::chars_format::scientific);
    std::string sci(buf, r.ptr);
    std::string sign;
    if (sci[0] == '-') {
        sign = "-";
        sci.erase(0, 1);
    }
    const size_t ep = sci.find('e');
    const int exp = std::stoi(sci.substr(ep + 1));
    std::string dig;
    for (size_t i = 0; i < ep; i++)
        if (sci[i] != '.') dig += sci[i];
    const float ax = std::fabs(x);
    std::string out;
    if (ax >= 1e-3f && ax < 1e7f) {
        if (exp >= 0) {
            std::string ip = dig.substr(0, std::min<size_t>(dig.size(), exp + 1));
            while ((int)ip.size() < exp + 1) ip += '0';
            std::string fp = (int)dig.size() > exp + 1 ? dig.substr(exp + 1) : "0";
            out = ip + "." + fp;
        } else {
            out = "0." + std::string(-exp - 1, '0') + dig;
        }
    } else {
        out = dig.substr(0, 1) + "." + (dig.size() > 1 ? dig.substr(1) : "0") + "E" + std::to_string(exp);
    }
    return sign + out;
}

// LongreadRecord.fromSAMRecord L120-150, literally: the walk over cigar.replaceAll("[0-9]+[IS]", "") split into cigartype ("[0-9]+") and
// cigarsize ("[A-Z]"); cigartype[i] is the operation BEFORE cigarsize[i], so the last operation is never looked at.  false: the reference
// throws (no block, a block index past the end, a size that is no integer)
inline bool walk_junctions(const uint8_t *bam, const smi_bam_record &r, std::vector<int2> &out) {
    static const char ops[] = "MIDNSHP=XBBBBBBB";
    std::string cig;
    struct Block {
        int64_t start, len;
    };
    std::vector<Block> blocks;  // AlignmentBlocks: M = X
    int64_t ref = (int64_t)r.pos + 1;
    for (int k = 0; k < r.n_cigar; k++) {
        uint32_t c;
        std::memcpy(&c, bam + r.cigar_off + 4ull * k, 4);
        const uint32_t op = c & 15, n = c >> 4;
        if (op == 0 || op == 7 || op == 8) {
            blocks.push_back({ref, n});
            ref += n;
        } else if (op == 2 || op == 3) {
            ref += n;
        }
        if (op == 1 || op == 4) continue;  // replaceAll("[0-9]+[IS]", "")
        cig += std::to_string(n);
        cig += ops[op];
    }
    if (blocks.empty()) return false;
    std::vector<std::string_view> type, size;  // cigar.split("[0-9]+"), cigar.split("[A-Z]")
    {
        std::string_view s(cig);
        size_t i = 0;
        type.push_back(std::string_view());  // the digits at position 0 give a leading ""
        while (i < s.size()) {
            while (i < s.size() && s[i] >= '0' && s[i] <= '9') i++;
            const size_t b = i;
            while (i < s.size() && !(s[i] >= '0' && s[i] <= '9')) i++;
            if (i > b) type.push_back(s.substr(b, i - b));
        }
        if (s.empty()) type.assign(1, std::string_view());
        size_t b = 0;
        for (size_t k = 0; k <= s.size(); k++)
            if (k == s.size() || (s[k] >= 'A' && s[k] <= 'Z')) {
                size.push_back(s.substr(b, k - b));
                b = k + 1;
            }
        while (!size.empty() && size.back().empty()) size.pop_back();
        if (s.empty()) size.assign(1, std::string_view());
    }
    int64_t s = blocks[0].start, e = blocks[0].start;
    std::vector<int64_t> xs, xe;
    size_t bi = 0;
    for (size_t i = 0; i < size.size(); i++) {
        if (bi >= blocks.size() || i >= type.size()) return false;
        const Block cur = blocks[bi];
        const std::string_view t = type[i];
        if (t == "M") bi++;
        if (t == "N") {
            xs.push_back(s);
            xe.push_back(e);
            s = cur.start;
        } else if (t == "D") {
            int32_t len;
            if (i == 0 || !jint(size[i - 1], len)) return false;
            if (len > 20) {  // a short intron minimap2 calls a deletion
                xs.push_back(s);
                xe.push_back(e);
                s = cur.start;
            }
        }
        if (t != "D") e = cur.start + cur.len - 1;
    }
    xs.push_back(s);
    xe.push_back(e);
    out.clear();
    for (size_t i = 1; i < xs.size(); i++) out.push_back(make_int2((int)xe[i - 1], (int)xs[i]));
    return true;
}

}  // namespace lr
}  // namespace smi
