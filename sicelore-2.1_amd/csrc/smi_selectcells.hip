// smi_selectcells.hip -- SelectValidCellBarcode: the cell list (barcodes.csv) from BarcodesAssigned.tsv.  Host only: no device
// code and no HIP header, so this unit also compiles alone with a plain C++ compiler (its one outside symbol is smi::set_error).
//
//   SelectValidCellBarcode.doWork                               org/ipmc/sicelore/programs/SelectValidCellBarcode.java:L39-92
//   BufferedReader.readLine (lines end at \n, \r\n or a lone \r; a last line without a terminator counts)            L57-58, L83
//   String.replaceAll(",", "") on the whole line, the barcode included                                               L60
//   String.split("\t"): leading empty fields stay, trailing empty fields go                                          L61
//   new Integer(String) = Integer.parseInt: [+-]?[0-9]+ inside the int range, nothing else                           L64-70
//   int / int before the conversion to double                                                                        L75
//
// The table is a few thousand rows (one per barcode that was assigned a read), so there is nothing here for the device.
//
// Deviation: a row the reference dies on -- fewer than four fields, a field parseInt rejects -- ends the
// reference's loop with a stack trace, an unclosed BufferedOutputStream and exit code 0.  Here the call returns 2, names the
// 1-based line and the reason, and gives no output at all.
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "sicelore_mi.h"

namespace smi {
void set_error(const std::string &msg);
}

namespace {

// Integer.parseInt(s, 10) with ASCII digits
bool parse_java_int(const char *s, size_t n, int32_t *out) {
    size_t i = 0;
    bool neg = false;
    if (n && (s[0] == '-' || s[0] == '+')) {
        neg = s[0] == '-';
        i = 1;
    }
    if (i == n) return false;
    int64_t v = 0;
    const int64_t limit = neg ? (int64_t)1 << 31 : ((int64_t)1 << 31) - 1;
    for (; i < n; i++) {
        if (s[i] < '0' || s[i] > '9') return false;
        v = v * 10 + (s[i] - '0');
        if (v > limit) return false;
    }
    *out = neg ? (v == ((int64_t)1 << 31) ? INT32_MIN : (int32_t)-v) : (int32_t)v;
    return true;
}

// Java's int / int: truncates toward zero, and Integer.MIN_VALUE / -1 wraps to Integer.MIN_VALUE (JLS 15.17.2)
int32_t java_div(int32_t a, int32_t b) {
    const int64_t q = (int64_t)a / (int64_t)b;
    return q > INT32_MAX ? INT32_MIN : (int32_t)q;
}

// String.split("\t") on [s, s + n): (offset, length) of every field, trailing empty fields dropped ("" gives one field, "\t" none)
void java_split_tabs(const char *s, size_t n, std::vector<std::pair<size_t, size_t>> &f) {
    f.clear();
    size_t start = 0;
    for (size_t i = 0; i <= n; i++)
        if (i == n || s[i] == '\t') {
            f.emplace_back(start, i - start);
            start = i + 1;
        }
    if (f.size() == 1) return;  // no tab at all: the string itself, an empty one too
    while (!f.empty() && f.back().second == 0) f.pop_back();
}

// the text of a field for a message: at most 40 bytes, anything outside printable ASCII as '?'
std::string shown(const char *s, size_t n) {
    std::string r(s, n < 40 ? n : 40);
    for (char &c : r)
        if ((unsigned char)c < 0x20 || (unsigned char)c > 0x7e) c = '?';
    return n > 40 ? r + "..." : r;
}

// one readLine(): false at the end of the text
bool read_line(const char *t, size_t n, size_t *pos, size_t *begin, size_t *len) {
    if (*pos >= n) return false;
    size_t i = *pos;
    while (i < n && t[i] != '\n' && t[i] != '\r') i++;
    *begin = *pos;
    *len = i - *pos;
    if (i < n) i += (t[i] == '\r' && i + 1 < n && t[i + 1] == '\n') ? 2 : 1;
    *pos = i;
    return true;
}

}  // namespace

extern "C" int smi_select_valid_cells(const char *tsv, size_t n, int32_t min_umi, double ed0ed1_ratio, char *out, size_t cap_out,
                                      size_t *n_out, char *removed, size_t cap_removed, size_t *n_removed, int64_t *counts,
                                      uint64_t *error_line) {
    if ((n && !tsv) || !n_out || !n_removed || !counts) {
        smi::set_error("smi_select_valid_cells: bad argument");
        return SMI_ERR_INVALID;
    }
    if (error_line) *error_line = 0;
    std::string kept_text, removed_text, line;
    std::vector<std::pair<size_t, size_t>> f;
    int64_t total = 0, kept = 0;
    size_t pos = 0, begin = 0, len = 0;
    uint64_t line_no = 1;
    size_t header_fields = 0;
    if (read_line(tsv, n, &pos, &begin, &len)) {  // the header (L57): skipped, only its width is kept for the message below
        java_split_tabs(tsv + begin, len, f);
        header_fields = f.size();
    }
    auto bad_row = [&](const std::string &why) {
        if (error_line) *error_line = line_no;
        smi::set_error("smi_select_valid_cells: line " + std::to_string(line_no) + ": " + why);
        return 2;
    };
    while (read_line(tsv, n, &pos, &begin, &len)) {
        line_no++;
        line.clear();
        for (size_t i = 0; i < len; i++)
            if (tsv[begin + i] != ',') line += tsv[begin + i];
        java_split_tabs(line.data(), line.size(), f);
        total++;
        if (f.size() < 4) {
            std::string why = std::to_string(f.size()) + (f.size() == 1 ? " field" : " fields") +
                              " where SelectValidCellBarcode reads four (barcode, reads, ED=0, ED=1)";
            if (header_fields == 3 && f.size() == 3)
                why += ": the table has no ED=1 column (it was written with --bcEditDistance 0)";
            return bad_row(why);
        }
        int32_t v[3];
        static const char *const NAME[3] = {"reads", "ED=0", "ED=1"};
        for (int k = 0; k < 3; k++) {
            const char *s = line.data() + f[k + 1].first;
            const size_t m = f[k + 1].second;
            if (k > 0 && m == 0) {  // L65-69: a present but empty ED=0 / ED=1 reads as 0
                v[k] = 0;
                continue;
            }
            if (!parse_java_int(s, m, &v[k]))
                return bad_row(std::string("field ") + std::to_string(k + 2) + " (" + NAME[k] + ") \"" + shown(s, m) +
                               "\" is not an int (Integer.parseInt)");
        }
        if (v[2] == 0) v[2] = 1;  // L72
        const std::string bc(line.data() + f[0].first, f[0].second);
        if (v[0] >= min_umi && (double)java_div(v[1], v[2]) >= ed0ed1_ratio) {
            kept++;
            kept_text += bc;
            kept_text += '\n';
        } else {
            removed_text += bc;
            removed_text += " barcode removed\t\t[";
            removed_text += line;
            removed_text += "]\n";
        }
    }
    counts[0] = total;
    counts[1] = kept;
    *n_out = kept_text.size();
    *n_removed = removed_text.size();
    if ((out && kept_text.size() > cap_out) || (removed && removed_text.size() > cap_removed)) {
        smi::set_error("smi_select_valid_cells: output buffer too small");
        return SMI_ERR_INVALID;
    }
    if (out && !kept_text.empty()) std::memcpy(out, kept_text.data(), kept_text.size());
    if (removed && !removed_text.empty()) std::memcpy(removed, removed_text.data(), removed_text.size());
    return SMI_OK;
}
