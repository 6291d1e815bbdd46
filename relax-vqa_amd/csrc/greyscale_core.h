// The greyscale screen (include/relax_hip.h: relax_greyscale_scan, relax_yuv_greyscale_scan): what one lane does with its
// pixels, the frame geometry and the record, with no HIP in it.  greyscale.hip compiles it for the device; greyscale_host.cpp
// compiles the same text for the host (librelax_greyscale_host.so for the CPU tests, and the stand-alone sanitizer program
// behind `make greyscale_san`), so the offsets a kernel lane uses are the offsets the CPU test walks.
#pragma once
#include <stdint.h>

#include "relax_hip.h"
#include "yuv_core.h"

#define GREY_HD YUV_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GREY_UNROLL _Pragma("unroll")   // the word arrays of a lane live in registers: every index must be a constant
#else
#define GREY_UNROLL
#endif

namespace grey {

constexpr int kRecordWords = RELAX_GREYSCALE_RECORD_WORDS;
constexpr int kStatusWord = 6;
constexpr int kLanePixels = 16;   // pixels of one unit: 48 bytes of BGR, or yuv_core.h's unit of a YUV frame
constexpr int kLaneUnits = 4;     // units one lane takes, kBlock apart, so that a wave's loads of one step are adjacent
constexpr int kBlock = 256;

// ---- the running extremes of one lane ----------------------------------------------------------------------------------------
// Per difference d = b-g, b-r, g-r (-255..255) three extremes are kept, each one instruction per pixel: the signed maximum, the
// signed minimum, and the maximum of d read as unsigned - under which every negative d beats every positive one and the
// negative d nearest to zero wins.  From them, exactly:
//     max |d|         = max(hi, -lo)
//     max (d mod 256) = max(hi if any d >= 0, 256 + (the negative d nearest to zero) if any d < 0)
struct Acc {
    int hi[3], lo[3];
    uint32_t um[3];
};

GREY_HD void init(Acc* a) {
    for (int q = 0; q < 3; ++q) a->hi[q] = -256, a->lo[q] = 256, a->um[q] = 0;
}

GREY_HD void add(Acc* a, int b, int g, int r) {
    const int d[3] = {b - g, b - r, g - r};
    GREY_UNROLL
    for (int q = 0; q < 3; ++q) {
        a->hi[q] = d[q] > a->hi[q] ? d[q] : a->hi[q];
        a->lo[q] = d[q] < a->lo[q] ? d[q] : a->lo[q];
        const uint32_t u = static_cast<uint32_t>(d[q]);
        a->um[q] = u > a->um[q] ? u : a->um[q];
    }
}

// -> m[0..2] the wrapped maxima, m[3..5] the absolute ones; a lane that saw no pixel gives zeros
GREY_HD void finish(const Acc& a, int32_t* m) {
    GREY_UNROLL
    for (int q = 0; q < 3; ++q) {
        const int32_t nearest = static_cast<int32_t>(a.um[q]);          // < 0 iff some d < 0
        const int pos = a.hi[q] > 0 ? a.hi[q] : 0;
        const int neg = nearest < 0 ? 256 + nearest : 0;
        m[q] = pos > neg ? pos : neg;
        const int ab = a.hi[q] > -a.lo[q] ? a.hi[q] : -a.lo[q];
        m[3 + q] = ab > 0 ? ab : 0;
    }
}

// ---- BGR frames ----------------------------------------------------------------------------------------------------------------
// A frame is H*W consecutive pixels; unit u holds pixels [16u, 16u + 16), bytes [48u, 48u + 48) of the frame.
// -> 0, or the number (1-based) of the offending argument: 1 H, 2 W
GREY_HD int check_size(int H, int W) {
    if (H < 1 || H > yuv::kMaxDim) return 1;
    if (W < 1 || W > yuv::kMaxDim) return 2;
    return 0;
}
GREY_HD int64_t pixels(int H, int W) { return static_cast<int64_t>(H) * W; }
GREY_HD int64_t units(int64_t npix) { return (npix + kLanePixels - 1) / kLanePixels; }
GREY_HD int64_t blocks(int64_t nunits) { return (nunits + kBlock * kLaneUnits - 1) / (kBlock * kLaneUnits); }
// the unit of lane `lane` of block `block` at step j
GREY_HD int64_t unit_of(int64_t block, int lane, int j) { return block * (kBlock * kLaneUnits) + j * kBlock + lane; }
// the 16-byte path: the frame's first byte at a 16-byte-aligned address (48 bytes per unit keep every unit aligned)
GREY_HD bool fast_path(uint64_t frame_addr) { return frame_addr % 16 == 0; }
// a unit may take three 16-byte loads iff all of its 16 pixels exist
GREY_HD bool unit_is_full(int64_t npix, int64_t unit) { return unit * kLanePixels + kLanePixels <= npix; }

GREY_HD int byte_of(const uint32_t* w, int i) { return static_cast<int>((w[i >> 2] >> ((i & 3) * 8)) & 255u); }

// 16 pixels as the 12 words of three 16-byte loads: b g r b | g r b g | r b g r ...
GREY_HD void unit_words(Acc* a, const uint32_t* w) {
    GREY_UNROLL
    for (int p = 0; p < kLanePixels; ++p) add(a, byte_of(w, 3 * p), byte_of(w, 3 * p + 1), byte_of(w, 3 * p + 2));
}

// any unit, a byte at a time; every index below npix
GREY_HD void unit_bytewise(Acc* a, const uint8_t* f, int64_t npix, int64_t unit) {
    const int64_t p0 = unit * kLanePixels;
    const int64_t p1 = p0 + kLanePixels < npix ? p0 + kLanePixels : npix;
    for (int64_t p = p0; p < p1; ++p) add(a, f[3 * p], f[3 * p + 1], f[3 * p + 2]);
}

// ---- YUV frames: yuv_core.h's plan, units, accesses and pixel arithmetic; the converted pixel goes into the extremes -------------
GREY_HD void yuv_unit_bytewise(Acc* a, const yuv::Plan& p, const yuv::Coef& k, const uint8_t* f, int64_t unit) {
    const yuv::Unit u = yuv::unit_at(p, unit);
    for (int r = u.r0; r < u.r0 + u.rows; ++r)
        for (int c = u.c0; c < u.c0 + u.cols; ++c) {
            int b, g, rr;
            yuv::pixel(k, f[yuv::y_at(p, r, c)], f[yuv::u_at(p, r, c)], f[yuv::v_at(p, r, c)], &b, &g, &rr);
            add(a, b, g, rr);
        }
}

// 16 pixels of one row from the words of its 16-byte Y load and the 16 chroma samples of these pixels (replicated already)
GREY_HD void yuv_row16(Acc* a, const yuv::Coef& k, const uint32_t* yw, const uint32_t* cu, const uint32_t* cv) {
    GREY_UNROLL
    for (int p = 0; p < kLanePixels; ++p) {
        int b, g, r;
        yuv::pixel(k, byte_of(yw, p), byte_of(cu, p), byte_of(cv, p), &b, &g, &r);
        add(a, b, g, r);
    }
}

// 8 chroma bytes (two words) -> each replicated once: 16 bytes in four words
GREY_HD void widen8(const uint32_t* in, uint32_t* o) {
    GREY_UNROLL
    for (int j = 0; j < 4; ++j) {
        const uint32_t h = (in[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
        const uint32_t x = h & 255u, y = h >> 8;
        o[j] = x | (x << 8) | (y << 16) | (y << 24);
    }
}

// 16 interleaved bytes U0 V0 U1 V1 ... (four words) -> the replicated U and V words
GREY_HD void split_nv12(const uint32_t* in, uint32_t* u, uint32_t* v) {
    GREY_UNROLL
    for (int j = 0; j < 4; ++j) {
        const uint32_t x = in[j];
        const uint32_t ua = x & 255u, va = (x >> 8) & 255u, ub = (x >> 16) & 255u, vb = x >> 24;
        u[j] = ua | (ua << 8) | (ub << 16) | (ub << 24);
        v[j] = va | (va << 8) | (vb << 16) | (vb << 24);
    }
}

// ---- the RELAX_YUVF_* formats: yuv_core.h's plan_ex, units, accesses and pixel_ex ---------------------------------------------------
GREY_HD void yuv_unit_bytewise_ex(Acc* a, const yuv::Plan& p, const yuv::Coef& k, const uint8_t* f, int64_t unit) {
    const yuv::Unit u = yuv::unit_at_ex(p, unit);
    for (int r = u.r0; r < u.r0 + u.rows; ++r)
        for (int c = u.c0; c < u.c0 + u.cols; ++c) {
            int b, g, rr;
            yuv::pixel_bytewise_ex(p, k, f, r, c, &b, &g, &rr);
            add(a, b, g, rr);
        }
}

// 16 pixels of one row from the words of a lane's segments (K: yuv::Kind)
template <class K>
GREY_HD void yuv_row16_ex(Acc* a, const yuv::Plan& p, const yuv::Coef& k, const uint32_t* lw, const uint32_t* cu, const uint32_t* cv) {
    GREY_UNROLL
    for (int px = 0; px < kLanePixels; ++px) {
        int b, g, r;
        K::pixel(p, k, lw, cu, cv, px, &b, &g, &r);
        add(a, b, g, r);
    }
}

// a frame may be read iff it lies inside src (yuv::item_in_range with a slot that always fits)
GREY_HD bool yuv_frame_in_range(const yuv::Plan& p, int64_t src_off, int64_t src_bytes) {
    return yuv::item_in_range(p, src_off, src_bytes, 0, p.out_bytes);
}
// the 16-byte path of a YUV frame: yuv::fast_path with a slot that is always aligned
GREY_HD bool yuv_fast_path(const yuv::Plan& p, uint64_t frame_addr) { return yuv::fast_path(p, frame_addr, 0); }

}  // namespace grey
