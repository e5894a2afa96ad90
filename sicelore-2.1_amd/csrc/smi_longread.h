// smi_longread.h -- the attribute helpers of the LongreadRecord.fromSAMRecord parsers (ComputeConsensus in smi_consensus.hip,
// IsoformMatrix in smi_isoform.hip): host only.
#pragma once
#include <cstdint>
#include <cstring>

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
inline int valid_tag(const char *t) { return t[0] > ' ' && t[0] <= '~' && t[1] > ' ' && t[1] <= '~' && t[2] == 0; }

// LongreadRecord L108-112: the first or the last CIGAR operation is S or H and longer than MAXCLIP
inline bool chimeric(uint32_t first, uint32_t last, int32_t max_clip) {
    auto clip = [&](uint32_t c) { return ((c & 15) == 4 || (c & 15) == 5) && (int64_t)(c >> 4) > (int64_t)max_clip; };
    return clip(first) || clip(last);
}

}  // namespace lr
}  // namespace smi
