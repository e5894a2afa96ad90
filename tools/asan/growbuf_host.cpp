// The grow-only buffer of sicelore-2.1_amd/csrc/smi_growbuf.h on a CPU, against a counting stand-in for the memory calls: allocation sizes
// per head-room rule, the no-grow path, a failed allocation, and need_keep's order of allocate / copy / free.
//   g++ -std=c++17 -fsanitize=address,undefined -Isicelore-2.1_amd/csrc tools/asan/growbuf_host.cpp -o growbuf_host && ./growbuf_host
// Exit code 0 and "growbuf_host: ok", or the line of the first check that failed.  tests/test_handle_cpu.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "smi_growbuf.h"

// every call in order: "a<bytes>" alloc, "A<bytes>" alloc refused, "f" release, "w" wait, "c<bytes>" copy_front
static std::vector<std::string> g_log;
static int g_live = 0;             // blocks allocated and not released
static bool g_refuse = false;      // the next alloc fails
static const void *g_copy_src = nullptr;

struct CountingMem {
    static int alloc(void **p, size_t bytes) {
        if (g_refuse) {
            g_refuse = false;
            g_log.push_back("A" + std::to_string(bytes));
            return 2;
        }
        g_log.push_back("a" + std::to_string(bytes));
        *p = std::malloc(bytes ? bytes : 1);
        g_live++;
        return 0;
    }
    static int release(void *p) {
        g_log.push_back("f");
        std::free(p);
        g_live--;
        return 0;
    }
    static int wait(int) {
        g_log.push_back("w");
        return 0;
    }
    static int copy_front(void *dst, const void *src, size_t bytes, int) {
        g_log.push_back("c" + std::to_string(bytes));
        g_copy_src = src;
        if (bytes) std::memcpy(dst, src, bytes);  // (under the sanitizer: the old block is still alive here)
        return 0;
    }
};

static std::string take_log() {
    std::string s;
    for (const std::string &e : g_log) s += (s.empty() ? "" : " ") + e;
    g_log.clear();
    return s;
}

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "growbuf_host: line %d: %s\n", __LINE__, #cond); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

// a rising, falling and rising sequence of requests: the block is allocated at `first`, kept, and regrown at `second`
template <unsigned DIV, size_t ADD>
static int sequence(size_t first, size_t second) {
    {
        smi::GrowBuf<CountingMem, DIV, ADD> b;
        CHECK(b.need(0) == 0 && b.p == nullptr && b.cap == 0 && take_log().empty());
        CHECK(b.need(1000) == 0 && b.cap == first && b.p && take_log() == "a" + std::to_string(first));
        const void *p = b.p;
        CHECK(b.need(10) == 0 && b.need(1000) == 0 && b.need(first) == 0 && b.need(10, 0) == 0 && b.need_keep(first, 10, 0) == 0);
        CHECK(b.p == p && b.cap == first && take_log().empty());  // enough: no call, no wait
        CHECK(b.need(first + 1) == 0 && b.cap == second && take_log() == "f a" + std::to_string(second));
        CHECK(b.need(first + 1, 0) == 0 && take_log().empty());
        CHECK(b.need(second + 1, 0) == 0 && take_log().substr(0, 4) == "w f ");  // the wait, on the grow path only and in front of the free
        CHECK(g_live == 1);
    }
    CHECK(take_log() == "f" && g_live == 0);  // the destructor
    return 0;
}

int main() {
    if (sequence<0, 0>(1000, 1001)) return 1;
    if (sequence<8, 0>(1125, 1126 + 1126 / 8)) return 1;
    if (sequence<4, 0>(1250, 1251 + 1251 / 4)) return 1;
    if (sequence<4, 4096>(1250 + 4096, 5347 + 5347 / 4 + 4096)) return 1;
    {  // a failed allocation leaves (null, 0), whatever was there, and the next call starts over
        smi::GrowBuf<CountingMem, 4> b;
        g_refuse = true;
        CHECK(b.need(100) == 2 && b.p == nullptr && b.cap == 0 && take_log() == "A125");
        CHECK(b.need(100) == 0 && b.cap == 125 && take_log() == "a125");
        g_refuse = true;
        CHECK(b.need(200, 0) == 2 && b.p == nullptr && b.cap == 0 && take_log() == "w f A250" && g_live == 0);
        CHECK(b.need(8) == 0 && b.cap == 10 && take_log() == "a10");
    }
    CHECK(take_log() == "f" && g_live == 0);
    {  // need_keep: the new block exists and holds the front before the old one goes
        smi::GrowBuf<CountingMem, 4> b;
        CHECK(b.need_keep(64, 0, 0) == 0 && b.cap == 80 && take_log() == "a80 c0");  // (nothing to free)
        std::memset(b.p, 0x5A, 80);
        const void *old = b.p;
        CHECK(b.need_keep(400, 48, 0) == 0 && b.cap == 500 && take_log() == "a500 c48 f" && g_copy_src == old && g_live == 1);
        const unsigned char *q = b.as<const unsigned char>();
        for (int k = 0; k < 48; k++) CHECK(q[k] == 0x5A);
        g_refuse = true;  // refused: the old block stays as it was
        old = b.p;
        CHECK(b.need_keep(4000, 48, 0) == 2 && b.p == old && b.cap == 500 && take_log() == "A5000" && g_live == 1);
    }
    CHECK(take_log() == "f" && g_live == 0);
    std::puts("growbuf_host: ok");
    return 0;
}
