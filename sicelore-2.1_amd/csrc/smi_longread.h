// smi_longread.h -- LongreadRecord.fromSAMRecord and the LongreadParser filter, once, for the programs that read molecule records:
// the attribute helpers, the CIGAR walk and the Java text rules (SNPMatrix in smi_snp.hip reads these too), the record reader (Reader),
// the filters of IsoformMatrix, ComputeConsensus, CollapseModel and FusionDetector on top of it (read_isoform, read_consensus,
// read_collapse, read_fusion) and the per-segment fan-out over host threads (read_segment).  Host code but for aux_size, which the
// kernels that walk attributes call too; no HIP call and no set_error, so that a plain C++ compiler builds it
// (tools/asan/longread_host.cpp runs it on a CPU).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include "sicelore_mi.h"

namespace smi {
namespace lr {

struct Aux {
    const uint8_t *p = nullptr;  // the field (tag, type, value)
    size_t n = 0;
};

// Why aux_size refuses an attribute; kAuxOk = 0
enum AuxBad : int { kAuxOk = 0, kAuxTruncated, kAuxShortArray, kAuxBadElement, kAuxBadType };

// The one rule for the bytes of the attribute at p (tag, type, value), host and device: *n = its size and kAuxOk, or why it is refused:
// it runs past end (a Z / H without NUL in front of end included), a B with fewer than the 8 bytes of its header, a B of an unknown
// element type, an unknown type.  Nothing at or behind end is read.
__host__ __device__ inline int aux_size(const uint8_t *p, const uint8_t *end, size_t *n) {
    const size_t left = (size_t)(end - p);
    if (left < 3) return kAuxTruncated;
    switch (p[2]) {
        case 'A': case 'c': case 'C': *n = 4; break;
        case 's': case 'S': *n = 5; break;
        case 'i': case 'I': case 'f': *n = 7; break;
        case 'Z': case 'H': {
#ifdef __HIP_DEVICE_COMPILE__
            const uint8_t *z = p + 3;
            while (z < end && *z) z++;
            if (z == end) return kAuxTruncated;
#else
            const uint8_t *z = (const uint8_t *)std::memchr(p + 3, 0, left - 3);
            if (!z) return kAuxTruncated;
#endif
            *n = (size_t)(z - p) + 1;
            break;
        }
        case 'B': {
            if (left < 8) return kAuxShortArray;
            size_t w;
            switch (p[3]) {
                case 'c': case 'C': w = 1; break;
                case 's': case 'S': w = 2; break;
                case 'i': case 'I': case 'f': w = 4; break;
                default: return kAuxBadElement;
            }
            *n = 8 + w * ((uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24);
            break;
        }
        default: return kAuxBadType;
    }
    return *n <= left ? kAuxOk : kAuxTruncated;
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

// Java's String.split(regex) for a one-character separator: trailing empty strings removed.  Into `out`, for a caller that splits once
// per record and keeps the vector's memory.
inline void jsplit(std::string_view s, char sep, std::vector<std::string_view> &out) {
    out.clear();
    size_t b = 0;
    for (size_t i = 0; i <= s.size(); i++)
        if (i == s.size() || s[i] == sep) {
            out.push_back(s.substr(b, i - b));
            b = i + 1;
        }
    while (!out.empty() && out.back().empty()) out.pop_back();
    if (s.empty()) out.assign(1, std::string_view());  // "".split(x) = [""]
}
inline std::vector<std::string_view> jsplit(std::string_view s, char sep) {
    std::vector<std::string_view> out;
    jsplit(s, sep, out);
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

// ---- the record reader -------------------------------------------------------------------------------------------------------------------
enum Tag { kCell, kUmi, kGene, kRn, kDe, kDf, kIso, kTe, kPs, kCs, kUs, kTags };

// the attributes a program captures: de and df always, the others as it names them
struct TagSet {
    uint16_t id[kTags] = {};  // the captured ones, in the order they were set
    uint8_t tag[kTags] = {};  // what id[i] is
    int n = 0;
    TagSet() {
        set(kDe, "de");
        set(kDf, "df");
    }
    TagSet &set(Tag k, const char *t) {
        id[n] = tag16(t);
        tag[n++] = (uint8_t)k;
        return *this;
    }
    uint16_t of(Tag k) const {
        for (int i = 0; i < n; i++)
            if (tag[i] == k) return id[i];
        return 0;
    }
    std::string text(Tag k) const { return std::string{(char)(of(k) & 255), (char)(of(k) >> 8)}; }
};

inline std::string_view read_name(const uint8_t *bam, const smi_bam_record &r) {
    return std::string_view((const char *)bam + r.name_off, r.l_read_name ? r.l_read_name - 1 : 0);
}

enum Outcome : uint8_t { kKept, kNull, kChimeric, kNoGene, kNoUmi, kMapq0, kLowRn, kNotListed, kError };

// what the four programs keep of a record, in two cache lines (the thread that appends the kept records reads what the workers wrote);
// the views point into the segment (bc: before the "-1" removal); the read's name is read_name(bam, r)
struct Record {
    Outcome what = kError;
    bool has_umi = false, has_it = false;
    float de = 1.0f;
    int32_t rn = 1;
    int32_t tx_start = 0, tx_end = 0;  // getAlignmentStart, getAlignmentEnd
    std::string_view bc, umi, gene, cdna, it;
    std::vector<int2> junc;
};

// The steps of fromSAMRecord over one record.  Every step that can fail returns false with out.what = kError and the reason in err; a
// filter calls them in its program's order and returns at the first false.
struct Reader {
    const uint8_t *bam;
    const smi_bam_record &r;
    const char *program;
    Record &out;
    std::string &err;
    Aux aux[kTags];
    uint32_t c0 = 0, c1 = 0;  // the first and the last CIGAR operation

    Reader(const uint8_t *bam_, const smi_bam_record &r_, const char *program_, Record &out_, std::string &err_)
        : bam(bam_), r(r_), program(program_), out(out_), err(err_) {
        out.what = kError;
    }
    bool fail(std::string why) {
        out.what = kError;
        err = std::move(why);
        return false;
    }
    bool bad(const Aux &a) {
        return fail(std::string("attribute ") + (char)a.p[0] + (char)a.p[1] + " of type " + (char)a.p[2] + " is not the type " + program + " reads");
    }
    void is(Outcome o) { out.what = o; }
    bool has(Tag k) const { return aux[k].p != nullptr; }

    // the attribute walk: a repeated tag keeps its last value (and type), as htsjdk reads it
    bool attributes(const TagSet &tg) {
        const uint8_t *p = bam + r.aux_off, *end = p + r.aux_len;
        while (p < end) {
            size_t n;
            if (aux_size(p, end, &n)) return fail("malformed attributes");
            const uint16_t t = (uint16_t)(p[0] | p[1] << 8);
            for (int k = 0; k < tg.n; k++)
                if (t == tg.id[k]) aux[tg.tag[k]] = Aux{p, n};
            p += n;
        }
        return true;
    }
    bool str(Tag k, std::string_view &v) {  // (String) getAttribute; absent: v stays
        const Aux &a = aux[k];
        if (!a.p) return true;
        if (a.p[2] != 'Z') return bad(a);
        v = std::string_view((const char *)a.p + 3, a.n - 4);
        return true;
    }
    bool integer(Tag k, int64_t &v) {  // (Integer) getAttribute; absent: v stays
        return !aux[k].p || aux_integer(aux[k], v) || bad(aux[k]);
    }
    bool rn() {  // L95
        int64_t v = 1;
        if (!integer(kRn, v)) return false;
        out.rn = (int32_t)v;
        return true;
    }
    bool de() {  // L92-94: de, else df, else 1; df is looked at only when de is absent
        for (Tag k : {kDe, kDf}) {
            if (!aux[k].p) continue;
            if (aux[k].p[2] != 'f') return bad(aux[k]);
            std::memcpy(&out.de, aux[k].p + 3, 4);
            break;
        }
        return true;
    }
    bool null() const { return !aux[kCell].p || (r.flag & 4); }  // L80
    bool cigar_ends() {
        if (r.n_cigar == 0) return fail("no CIGAR");
        std::memcpy(&c0, bam + r.cigar_off, 4);
        std::memcpy(&c1, bam + r.cigar_off + 4 * ((size_t)r.n_cigar - 1), 4);
        return true;
    }
    bool clipped(int32_t max_clip) const { return chimeric(c0, c1, max_clip); }  // L108-112
    bool junctions(std::vector<int2> &junc) {                                    // L120-150
        return walk_junctions(bam, r, junc) || fail("the CIGAR walk runs past the alignment blocks");
    }
    void alignment() {
        int64_t ref_len = 0;
        for (int k = 0; k < r.n_cigar; k++) {
            uint32_t c;
            std::memcpy(&c, bam + r.cigar_off + 4ull * k, 4);
            const uint32_t op = c & 15;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += c >> 4;
        }
        out.tx_start = r.pos + 1;
        out.tx_end = (int32_t)(r.pos + ref_len);
    }
    bool no_gene() const { return !aux[kGene].p || out.gene.empty() || out.gene == "undef"; }  // LongreadParser L101
    bool mapq0_secondary() const { return r.mapq == 0 && (r.flag & 0x900); }                   // LongreadParser L105-112
};

// ---- the four programs: the order of the casts and of the tests is each program's own ----------------------------------------------------

// IsoformMatrix: tags cell, umi, gene, rn
inline void read_isoform(const uint8_t *bam, const smi_bam_record &r, const TagSet &tg, int32_t max_clip, bool mapqv0, Record &out,
                         std::string &err) {
    Reader rd(bam, r, "IsoformMatrix", out, err);
    if (!rd.attributes(tg)) return;
    if (!rd.str(kGene, out.gene) || !rd.str(kCell, out.bc) || !rd.str(kUmi, out.umi)) return;  // L75-77: the casts come first
    if (rd.null()) return rd.is(kNull);
    if (!rd.de() || !rd.rn()) return;
    if (!rd.cigar_ends()) return;
    if (!rd.junctions(out.junc)) return;  // (a failing walk is an error for a chimeric record too)
    if (rd.clipped(max_clip)) return rd.is(kChimeric);
    if (rd.no_gene()) return rd.is(kNoGene);
    if (!rd.has(kUmi)) return rd.is(kNoUmi);
    if (!mapqv0 && rd.mapq0_secondary()) return rd.is(kMapq0);
    rd.is(kKept);
}

// ComputeConsensus: tags cell, umi, gene, rn, te, ps, cs, us.  The cDNA is cs, else us cut at te and ps (L116-135).
inline void read_consensus(const uint8_t *bam, const smi_bam_record &r, const TagSet &tg, int32_t max_clip, bool mapqv0, Record &out,
                           std::string &err) {
    Reader rd(bam, r, "ComputeConsensus", out, err);
    if (!rd.attributes(tg)) return;
    if (!rd.str(kGene, out.gene) || !rd.str(kCell, out.bc) || !rd.str(kUmi, out.umi)) return;  // L75-81: the casts come first
    if (rd.null()) return rd.is(kNull);
    if (!rd.de() || !rd.rn()) return;  // (rn is not used further)
    if (!rd.cigar_ends()) return;
    if (rd.clipped(max_clip)) return rd.is(kChimeric);  // before the cDNA is cut; the junction walk does not run
    if (!rd.str(kCs, out.cdna)) return;
    if (!rd.has(kCs)) {
        std::string_view us;
        if (!rd.str(kUs, us)) return;
        if (!rd.has(kUs)) return (void)rd.fail("neither " + tg.text(kCs) + " nor " + tg.text(kUs));
        int64_t tso = 0, pa = 0;
        if (!rd.integer(kTe, tso) || !rd.integer(kPs, pa)) return;
        const int64_t len = (int64_t)us.size();
        const int64_t e = (pa != 0 && pa < len - 1) ? pa : len - 1;
        if (tso < e && tso < 0) return (void)rd.fail(tg.text(kTe) + " " + std::to_string(tso) + " is outside " + tg.text(kUs));  // substring throws
        out.cdna = tso < e ? us.substr((size_t)tso, (size_t)(e - tso)) : us;
    }
    if (!rd.has(kUmi)) return rd.is(kNoUmi);  // LongreadParser L103
    if (!mapqv0 && rd.mapq0_secondary()) return rd.is(kMapq0);
    rd.is(kKept);
}

// CollapseModel: tags cell, umi, gene, rn, iso.  listed(barcode): the cell list's contains().
template <class Listed>
inline void read_collapse(const uint8_t *bam, const smi_bam_record &r, const TagSet &tg, int32_t max_clip, int32_t rn_min, Listed &&listed,
                          Record &out, std::string &err) {
    Reader rd(bam, r, "CollapseModel", out, err);
    if (!rd.attributes(tg)) return;
    // loader L157-161: every cast, RN's too, comes before anything else, for every record
    std::string_view umi;  // (cast, not kept)
    if (!rd.str(kCell, out.bc) || !rd.str(kUmi, umi) || !rd.str(kGene, out.gene) || !rd.str(kIso, out.it)) return;
    out.has_it = rd.has(kIso);
    if (!rd.rn()) return;
    if (rd.null() || r.ref_id < 0) return rd.is(kNull);  // (a record on no sequence is in no query)
    if (!rd.de()) return;
    if (!rd.cigar_ends()) return;
    if (!rd.junctions(out.junc)) return;  // the walk runs before the filter
    rd.alignment();
    // loader L167-170
    if (r.mapq == 0) return rd.is(kMapq0);
    if (rd.clipped(max_clip)) return rd.is(kChimeric);
    if (out.rn < rn_min) return rd.is(kLowRn);
    if (!listed(out.bc)) return rd.is(kNotListed);
    if (rd.no_gene()) return rd.is(kNoGene);
    rd.is(kKept);
}

// FusionDetector (FusionDetector.java L63-67): tags BC U8 GE RN, MAXCLIP 10000, gene mandatory, UMI not, mapq-0 records kept when primary
inline void read_fusion(const uint8_t *bam, const smi_bam_record &r, const TagSet &tg, int32_t max_clip, Record &out, std::string &err) {
    Reader rd(bam, r, "FusionDetector", out, err);
    if (!rd.attributes(tg)) return;
    if (!rd.str(kGene, out.gene) || !rd.str(kCell, out.bc) || !rd.str(kUmi, out.umi)) return;  // L75-77: the casts come first
    out.has_umi = rd.has(kUmi);
    if (rd.null()) return rd.is(kNull);
    if (!rd.de() || !rd.rn()) return;
    if (!rd.cigar_ends()) return;
    std::vector<int2> junc;  // (not kept)
    if (!rd.junctions(junc)) return;  // the walk runs for every record that is not null
    if (rd.clipped(max_clip)) return rd.is(kChimeric);
    if (rd.no_gene()) return rd.is(kNoGene);
    if (rd.mapq0_secondary()) return rd.is(kMapq0);
    rd.is(kKept);
}

// ---- one segment ----------------------------------------------------------------------------------------------------------------------
// The records of a segment.  Each is constructed by the thread that reads it: the array's pages are then first touched by the workers and
// not one after the other by the caller, which was close to half of a segment's time when the caller built a std::vector of them.
class Records {
    Record *p_ = nullptr;
    size_t n_ = 0;

   public:
    Records() = default;
    explicit Records(size_t n) : p_(n ? (Record *)::operator new(n * sizeof(Record)) : nullptr), n_(n) {}
    Records(Records &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    Records &operator=(Records &&o) noexcept {
        std::swap(p_, o.p_), std::swap(n_, o.n_);
        return *this;
    }
    ~Records() {  // (read_segment has constructed every one by the time it returns)
        for (size_t i = 0; i < n_; i++) p_[i].~Record();
        ::operator delete(p_);
    }
    Record *raw(size_t i) { return p_ + i; }
    const Record &operator[](size_t i) const { return p_[i]; }
    const Record *begin() const { return p_; }
    const Record *end() const { return p_ + n_; }
    size_t size() const { return n_; }
};

struct Segment {
    Records recs;
    int32_t first_error = -1;  // the first record in file order whose outcome is kError
    std::string error;         // why that record failed
    std::string refused;       // not empty: a record lies outside the segment and nothing was read
};

// read(bam, recs[i], out, err) for every record of the segment, on up to n_threads host threads; fn: the caller's name, for `refused`
template <class Read>
Segment read_segment(const char *fn, const uint8_t *bam, size_t n_bam, const smi_bam_record *recs, int32_t n, int n_threads, Read &&read) {
    Segment seg;
    for (int32_t i = 0; i < n; i++) {
        const smi_bam_record &r = recs[i];
        if (r.name_off + r.l_read_name > n_bam || r.cigar_off + 4ull * r.n_cigar > n_bam || r.aux_off + r.aux_len > n_bam) {
            seg.refused = std::string(fn) + ": record " + std::to_string(i) + " lies outside the segment";
            return seg;
        }
    }
    seg.recs = Records((size_t)n);
    const int nt = std::max(1, std::min<int>(n_threads, (n + 4095) / 4096));
    struct Failed {  // per thread: the first failing record of its slice
        int32_t i = -1;
        std::string why;
    };
    std::vector<Failed> failed(nt);
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++)
        th.emplace_back([&, t] {
            std::string err;
            for (int32_t i = (int32_t)((int64_t)n * t / nt); i < (int32_t)((int64_t)n * (t + 1) / nt); i++) {
                Record *out = new (seg.recs.raw(i)) Record;
                read(bam, recs[i], *out, err);
                if (out->what == kError && failed[t].i < 0) failed[t] = Failed{i, err};
            }
        });
    for (auto &x : th) x.join();
    for (int t = 0; t < nt && seg.first_error < 0; t++) {
        seg.first_error = failed[t].i;
        seg.error = std::move(failed[t].why);
    }
    return seg;
}

}  // namespace lr
}  // namespace smi
