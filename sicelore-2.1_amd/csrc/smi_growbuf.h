// smi_growbuf.h -- the grow-only scratch buffer a context owns (smi_internal.h gives it its device and its pinned-host form).  Nothing here
// names a device: a plain C++ compiler builds it against a counting stand-in for the memory calls (tools/asan/growbuf_host.cpp).
#pragma once
#include <cstddef>

namespace smi {

// A block of at least the size last asked for, freed by its destructor.  Mem says where the block lives, as static functions that report
// their own failures and return 0 (SMI_OK) or an error code:
//   int alloc(void **p, size_t bytes)      int release(void *p)
//   int wait(S stream)                     -- what a caller with work in flight on the block passes through need(bytes, stream)
//   int copy_front(void *dst, const void *src, size_t bytes, S stream)   -- queue the copy (bytes may be 0), then wait for the stream
// Head-room is part of the type: a block that has to grow is allocated as bytes + bytes / DIV + ADD (DIV 0: nothing to spare).
template <class Mem, unsigned DIV = 0, size_t ADD = 0>
struct GrowBuf {
    void *p = nullptr;
    size_t cap = 0;  // bytes
    GrowBuf() = default;
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    ~GrowBuf() { if (p) (void)Mem::release(p); }
    template <class T>
    T *as() const { return static_cast<T *>(p); }  // the block as what its reader takes it for, said at the site
    static constexpr size_t grown(size_t bytes) { return bytes + bytes / (DIV ? DIV : 1) * (DIV != 0) + ADD; }

    // Room for `bytes`.  Enough already: the compare and nothing else (no call, no wait).  Otherwise the old block is freed and a new one
    // allocated; the contents are lost, and a failure leaves the buffer empty (null, 0).
    int need(size_t bytes) { return cap >= bytes ? 0 : grow(bytes); }
    // ... for a block that work queued on `stream` may still read or write: the grow path waits for the stream before it frees
    template <class S>
    int need(size_t bytes, S stream) {
        if (cap >= bytes) return 0;
        if (int rc = Mem::wait(stream)) return rc;
        return grow(bytes);
    }
    // ... keeping the first keep_bytes: the new block exists and holds them before the old one is freed (a failed allocation leaves the old
    // block as it was).  Waits for `stream` on the grow path.
    template <class S>
    int need_keep(size_t bytes, size_t keep_bytes, S stream) {
        if (cap >= bytes) return 0;
        void *fresh = nullptr;
        if (int rc = Mem::alloc(&fresh, grown(bytes))) return rc;
        if (int rc = Mem::copy_front(fresh, p, keep_bytes, stream)) {
            (void)Mem::release(fresh);
            return rc;
        }
        void *old = p;
        p = fresh;
        cap = grown(bytes);
        return old ? Mem::release(old) : 0;
    }

private:
    int grow(size_t bytes) {
        void *old = p;
        p = nullptr;
        cap = 0;
        if (old)
            if (int rc = Mem::release(old)) return rc;
        if (int rc = Mem::alloc(&p, grown(bytes))) {
            p = nullptr;
            return rc;
        }
        cap = grown(bytes);
        return 0;
    }
};

}  // namespace smi
