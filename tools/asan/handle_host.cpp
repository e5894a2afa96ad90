// The host plumbing of sicelore-2.1_amd/csrc/smi_handle.h on a CPU, as the handles call it: the CellList reader, the refFlat line
// reader, the size protocol of a text getter and the error_read body.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Isicelore-2.1_amd/csrc tools/asan/handle_host.cpp
//   (add -fsanitize=address,undefined to the g++ line for a sanitizer run)
//   handle_host cells FILE              one `cell <text>` line per line of the list, in file order, "-1" removed
//   handle_host refflat WHO STRAND FILE the lines of FILE cut at \n as the parse_model functions cut them, STRAND 1 = with CollapseModel's
//                                       strand check: `kept <line> <gene> <tx> <strand> <five integers> <starts,> <ends,>`, `dropped <line>`,
//                                       or `bad <error text>`, which ends the run as it ends parse_model
//   handle_host getter FILE             the protocol over FILE's bytes: `size <rc> <n>`, `short <rc> <n> <untouched 0/1>` (cap one short, not
//                                       run for an empty text), `exact <rc> <n> <equal 0/1> <byte behind untouched 0/1>`
//   handle_host error_read NAME RECORD  cap 0, 1, 4 and 64: `<cap> <rc> <record> <bytes written up to the NUL, or - when none> <rest untouched 0/1>`
// Fields are separated by tabs.  tests/test_handle_cpu.py builds and runs it and compares with the Python models.
#include <cstdio>
#include <fstream>
#include <iterator>

#include "smi_handle.h"

using namespace smi;

static std::string join(const std::vector<int32_t> &v) {
    std::string s;
    for (int32_t x : v) s += std::to_string(x) + ",";
    return s;
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "error_read" && argc == 4) {
        const std::string name = argv[2];
        for (size_t cap : {(size_t)0, (size_t)1, (size_t)4, (size_t)64}) {
            std::vector<char> buf(64, '#');
            int64_t record = -7;
            const int rc = handle::error_read(name, std::atoll(argv[3]), cap ? buf.data() : nullptr, cap, &record);
            size_t nul = 0;
            while (nul < buf.size() && buf[nul]) nul++;
            const bool wrote = cap != 0;
            bool rest = true;
            for (size_t i = wrote ? nul + 1 : 0; i < buf.size(); i++) rest = rest && buf[i] == '#';
            std::printf("%zu\t%d\t%lld\t%s\t%d\n", cap, rc, (long long)record, wrote ? std::string(buf.data(), nul).c_str() : "-", (int)rest);
        }
        return 0;
    }
    const char *path = mode == "refflat" && argc == 5 ? argv[4] : (mode == "cells" || mode == "getter") && argc == 3 ? argv[2] : nullptr;
    if (!path) {
        std::fprintf(stderr, "usage: handle_host cells FILE | refflat WHO STRAND FILE | getter FILE | error_read NAME RECORD\n");
        return 2;
    }
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        std::fprintf(stderr, "handle_host: cannot open %s\n", path);
        return 2;
    }
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (mode == "cells") {
        for (const std::string &c : handle::cell_list(text.data(), text.size())) std::printf("cell\t%s\n", c.c_str());
    } else if (mode == "refflat") {
        handle::RefFlatLine L;
        std::string err;
        int64_t lineno = 0;
        for (size_t b = 0; b < text.size();) {
            size_t e = b;
            while (e < text.size() && text[e] != '\n') e++;
            const int kind = handle::refflat_line(argv[2], std::string_view(text.data() + b, e - b), ++lineno, argv[3][0] == '1', L, err);
            b = e + 1;
            if (kind == handle::kLineBad) {
                std::printf("bad\t%s\n", err.c_str());
                break;
            }
            if (kind == handle::kLineDropped)
                std::printf("dropped\t%lld\n", (long long)lineno);
            else
                std::printf("kept\t%lld\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n", (long long)lineno, std::string(L.gene).c_str(), std::string(L.tx).c_str(),
                            std::string(L.strand).c_str(), L.tx_start, L.tx_end, L.cds_start, L.cds_end, L.n_exon, join(L.xs).c_str(), join(L.xe).c_str());
        }
    } else {
        size_t n = ~(size_t)0;
        int rc = handle::get_text(text, nullptr, 0, &n);
        std::printf("size\t%d\t%zu\n", rc, n);
        std::vector<uint8_t> buf(text.size() + 1, '#');
        if (!text.empty()) {
            n = ~(size_t)0;
            rc = handle::get_text(text, buf.data(), text.size() - 1, &n);
            bool untouched = true;
            for (uint8_t c : buf) untouched = untouched && c == '#';
            std::printf("short\t%d\t%zu\t%d\n", rc, n, (int)untouched);
        }
        n = ~(size_t)0;
        rc = handle::get_text(text, buf.data(), text.size(), &n);
        std::printf("exact\t%d\t%zu\t%d\t%d\n", rc, n, (int)(std::memcmp(buf.data(), text.data(), text.size()) == 0), (int)(buf[text.size()] == '#'));
    }
    return 0;
}
