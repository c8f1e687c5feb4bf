// sized_out.h — the host side of an entry whose output's size is known only after a first pass on the device (K13, K16, K17,
// K20, K21, K22, K23): measure, scan, read the totals back, get the buffer, print.  Host code only.
#pragma once

#include "dyd_common.h"

namespace dyd {

// The context's scratch for the launches of one function on `st`: released (release_scratch records its event) when the
// lease leaves scope, on every way out, so after the function's last launch.
struct ScratchLease {
    hipStream_t st;
    bool held = false;
    explicit ScratchLease(hipStream_t s) : st(s) {}
    ScratchLease(const ScratchLease &) = delete;
    ~ScratchLease() {
        if (held) release_scratch(st);
    }
    int get(size_t bytes, void **out) {
        const int rc = get_scratch(bytes, out, st);
        held = rc == DYD_OK;
        return rc;
    }
};

struct ReadWord {
    int64_t *dst;          // host
    const int64_t *src;    // device
};

// The status of the launches so far, then every 8-byte device word into its host word, then the wait for st: the first error
// wins and is reported as "<kernel>: <step> failed".
inline int read_totals(const char *kernel, const char *step, std::initializer_list<ReadWord> words, hipStream_t st) {
    hipError_t e = hipGetLastError();
    for (const ReadWord &w : words)
        if (e == hipSuccess) e = hipMemcpyAsync(w.dst, w.src, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) return DYD_OK;
    set_error("%s: %s failed: %s", kernel, step, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? DYD_ERR_OOM : DYD_ERR_HIP;
}

// what a sized output is called in a message, and the bytes of one element
struct SizedName {
    const char *kernel, *what, *unit;
    size_t elem;
};

// Where a sized output goes: the caller's buffer (p may be NULL: measure only) of `cap` elements, or a buffer the library
// allocates in `st` at exactly the total.  K7 stays out: its single-pass kernels need the buffer at launch and detect a short
// one themselves.
struct SizedOut {
    SizedName name;
    void *p;
    int64_t cap;
    bool own;
    hipStream_t st;
    DevBuf buf;

    SizedOut(const SizedName &n, void *ptr, int64_t cap_elems) : name(n), p(ptr), cap(cap_elems), own(false), st(nullptr) {}
    SizedOut(const SizedName &n, hipStream_t stream) : name(n), p(nullptr), cap(0), own(true), st(stream) {}
    SizedOut(const SizedOut &) = delete;

    // the total is known: p is the buffer afterwards (NULL with DYD_OK: measure only).  A caller's buffer below the total is
    // DYD_ERR_RANGE; this is the one place that formats the message.
    int get(int64_t total) {
        if (own) {
            const int rc = buf.alloc(name.elem * (size_t)total, st);
            p = buf.p;
            cap = total;
            return rc;
        }
        if (p && total > cap) {
            set_error("%s: %s buffer too small (%lld %s needed, %lld given)", name.kernel, name.what, (long long)total, name.unit,
                      (long long)cap);
            return DYD_ERR_RANGE;
        }
        return DYD_OK;
    }
    template <class T>
    T *as() { return static_cast<T *>(p); }
};

}  // namespace dyd
