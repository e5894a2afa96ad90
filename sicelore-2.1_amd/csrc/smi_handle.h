// smi_handle.h -- the host plumbing the per-program handles share (smi_isoform.hip, smi_snp.hip, smi_collapse.hip, smi_fusion.hip,
// smi_consensus.hip, smi_moltag.hip): the body of a text getter, the body of an error_read, the CellList reader and the refFlat line
// reader of IsoformMatrix and CollapseModel.  The entry points keep their own argument and state checks and their own error texts.
// Host only: no HIP call and no set_error (an error comes back as text), so that a plain C++ compiler builds it
// (tools/asan/handle_host.cpp runs it on a CPU).
#pragma once
#include "smi_longread.h"

namespace smi {
namespace handle {

// A text getter's size protocol: *n_out = size always; out == NULL asks for the size alone; 1 = cap is too small (out untouched).
inline int get_text(std::string_view s, uint8_t *out, size_t cap, size_t *n_out) {
    *n_out = s.size();
    if (!out) return SMI_OK;
    if (cap < s.size()) return 1;
    std::memcpy(out, s.data(), s.size());
    return SMI_OK;
}

// The read a failed segment named: its name cut to cap - 1 bytes and a NUL (cap 0: nothing is written), *record either way.
inline int error_read(const std::string &read, int64_t error_record, char *name, size_t cap, int64_t *record) {
    *record = error_record;
    if (cap) {
        const size_t k = std::min(cap - 1, read.size());
        std::memcpy(name, read.data(), k);
        name[k] = 0;
    }
    return SMI_OK;
}

// CellList: every line (readLine: \n, \r\n or \r) with "-1" removed, in file order
inline std::vector<std::string> cell_list(const char *csv, size_t n_csv) {
    std::vector<std::string> cells;
    size_t b = 0;
    while (b < n_csv) {
        size_t e = b;
        while (e < n_csv && csv[e] != '\n' && csv[e] != '\r') e++;
        cells.push_back(lr::drop_minus1(std::string_view(csv + b, e - b)));
        if (e < n_csv && csv[e] == '\r' && e + 1 < n_csv && csv[e + 1] == '\n') e++;
        b = e + 1;
    }
    return cells;
}

struct RefFlatLine {  // the views point into the line
    std::string_view gene, tx, strand;
    int32_t tx_start, tx_end, cds_start, cds_end, n_exon;  // fields 5 .. 9
    std::vector<int32_t> xs, xe;                            // exon starts (as written, 0-based) and ends; xe may be the longer
};
enum { kLineKept = 0, kLineDropped = 1, kLineBad = 2 };

// One refFlat line (cut at \n; a trailing \r is dropped as BufferedReader.readLine does) as UCSCRefFlatParser.parseLine reads it.
// kLineDropped: its exon bases come to 0 in int arithmetic.  kLineBad: err = "<who>: REFFLAT line <lineno>: <why>".
// check_strand: CollapseModel's rule that field 4 is +, - or .
inline int refflat_line(const char *who, std::string_view line, int64_t lineno, bool check_strand, RefFlatLine &L, std::string &err) {
    if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
    const auto f = lr::jsplit(line, '\t');
    auto fail = [&](const std::string &why) {
        err = std::string(who) + ": REFFLAT line " + std::to_string(lineno) + ": " + why;
        return (int)kLineBad;
    };
    if (f.size() < 11) return fail("has " + std::to_string(f.size()) + " fields, at least 11 are needed");
    if (check_strand && f[3] != "+" && f[3] != "-" && f[3] != ".") return fail("field 4 is no strand (+, - or .)");
    int32_t *const v[] = {&L.tx_start, &L.tx_end, &L.cds_start, &L.cds_end, &L.n_exon};
    for (int k = 4; k <= 8; k++)
        if (!lr::jint(f[k], *v[k - 4])) return fail("field " + std::to_string(k + 1) + " is not an integer");
    L.xs.clear();
    L.xe.clear();
    for (int k = 9; k <= 10; k++) {
        std::string_view s = f[k];
        while (!s.empty() && s.back() == ',') s.remove_suffix(1);  // StringUtils.stripEnd(str, ",")
        for (auto t : lr::jsplit(s, ',')) {
            int32_t x;
            if (!lr::jint(t, x)) return fail("field " + std::to_string(k + 1) + " is not a list of integers");
            (k == 9 ? L.xs : L.xe).push_back(x);
        }
    }
    if (L.xe.size() < L.xs.size()) return fail("fewer exon ends than exon starts");
    int64_t bases = 0;
    for (size_t i = 0; i < L.xs.size(); i++) bases += (int64_t)L.xe[i] - L.xs[i];
    if ((int32_t)bases == 0) return kLineDropped;  // parseLine: getExonBases() == 0 -> dropped (int arithmetic)
    L.gene = f[0];
    L.tx = f[1];
    L.strand = f[3];
    return kLineKept;
}

}  // namespace handle
}  // namespace smi
