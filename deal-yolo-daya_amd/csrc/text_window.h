// text_window.h — the window of a text that one print workgroup fills in LDS and streams out (K16, K20; the host side also K13).
//
// A text of `total` bytes at address `text` is cut into windows of WINDOW bytes (a multiple of 16) that are aligned to 16
// bytes of the text's address: with phase = text & 15, window t holds the text bytes [t * WINDOW - phase, (t + 1) * WINDOW -
// phase) within [0, total), so neighbouring workgroups share no 16-byte chunk.  k13_print_kernel and k17_print_kernel keep
// their own copies of this code, written out: every helper here moves their register allocation.  K7's k7_flush
// is funnel-shifted and not this.
#pragma once

#include "dyd_common.h"
#include "round6.h"

namespace dyd {

struct TextWindows {
    int64_t phase, count;
};

// the phase of a text's address and the number of its windows
inline TextWindows text_windows(const void *text, int64_t total, int64_t window) {
    const int64_t phase = (int64_t)(reinterpret_cast<uintptr_t>(text) & 15u);
    return TextWindows{phase, ceil_div(total + phase, window)};
}

#if defined(__HIPCC__)
struct TextWindow {
    uint8_t *img;             // the window's image in LDS, 16-byte aligned
    int64_t base, wlo, whi;   // the text byte at img[0]; the window's bytes of the text

    // text byte a, dropped outside the window
    __device__ __forceinline__ void put(int64_t a, uint8_t c) const {
        if (a >= wlo && a < whi) img[a - base] = c;
    }
    // a class id >= 0 in its cd = k13_digits decimal digits at [a, a + cd)
    __device__ __forceinline__ void class_id(int64_t a, int32_t cid, int cd) const {
        uint32_t v = (uint32_t)cid;
        for (int k = cd - 1; k >= 0; --k) {
            const uint32_t d = v / 10u;
            put(a + k, (uint8_t)('0' + (v - d * 10u)));
            v = d;
        }
    }
    // " %.6f" of n(v) at [a, a + 9)
    __device__ __forceinline__ void field(int64_t a, double v) const {
        const uint64_t d = k13_num8(v);
        put(a, ' ');
#pragma unroll
        for (int k = 0; k < 8; ++k) put(a + 1 + k, (uint8_t)(d >> (8 * k)));
    }
    // stream the window out: text + base is 16-byte aligned; chunks cut by the text's ends go byte by byte
    template <int WINDOW, int BLOCK>
    __device__ __forceinline__ void flush(uint8_t *__restrict__ text) const {
        for (int64_t c = threadIdx.x; c < WINDOW / 16; c += BLOCK) {
            const int64_t a = base + 16 * c;
            if (a + 16 <= wlo || a >= whi) continue;
            if (a >= wlo && a + 16 <= whi) {
                *reinterpret_cast<uint4 *>(text + a) = *reinterpret_cast<const uint4 *>(img + 16 * c);
            } else {
                for (int k = 0; k < 16; ++k)
                    if (a + k >= wlo && a + k < whi) text[a + k] = img[16 * c + k];
            }
        }
    }
};

// window `block` of a text of `total` bytes
__device__ __forceinline__ TextWindow text_window(uint8_t *img, int64_t block, int64_t window, int64_t phase, int64_t total) {
    const int64_t base = block * window - phase;
    return TextWindow{img, base, max(base, (int64_t)0), min(base + window, total)};
}
#endif

}  // namespace dyd
