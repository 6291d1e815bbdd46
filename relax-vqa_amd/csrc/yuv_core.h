// Raw YUV frames -> BGR: frame layout, per-item bounds and the integer colour arithmetic of relax_yuv_to_bgr and, for the
// RELAX_YUVF_* formats (10 / 12-bit, packed 4:2:2, 4:1:1, 4:1:0, NV21), of relax_yuv_to_bgr_ex (include/relax_hip.h), with no HIP
// in it.  yuv.hip and greyscale.hip compile it for the device; yuv_host.cpp and yuv_ex_host.cpp compile the same text for the
// host (the stand-alone sanitizer programs behind `make sanitize_yuv` and `make sanitize_yuv_ex`), so the offsets a kernel lane
// uses are the offsets the CPU tests walk.
#pragma once
#include <stdint.h>

#include "relax_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define YUV_HD __host__ __device__ inline
#else
#define YUV_HD inline
#endif

namespace yuv {

// largest W or H taken (a stated limit; every offset below is int64, the per-pixel products fit int32 at any size)
constexpr int kMaxDim = RELAX_YUV_MAX_DIM;

// ---- formats ------------------------------------------------------------------------------------------
// The one table of RELAX_YUVF_* (relax_yuv_format_info hands it to the Python layer): how a sample is stored and where.
constexpr int kPlanar = RELAX_YUV_PACKING_PLANAR, kSemiPlanar = RELAX_YUV_PACKING_SEMIPLANAR, kPacked = RELAX_YUV_PACKING_PACKED;
constexpr int kMaxDepth = 12;   // with s = depth - 8 <= 4 every sum of pixel_ex() fits int32 (tests/test_yuv_ex_cpu.py evaluates the extremes in int64)

struct Format {
    int sb;               // bytes per sample: 1, or 2 (little endian)
    int depth;            // 8, 10 or 12: the sample is (word >> shift) & (2^depth - 1)
    int shift;            // 0: the value sits in the low bits (higher bits masked off); 6 for P010: the high 10 bits
    int hshift, vshift;   // 0..2
    int packing;          // kPlanar, kSemiPlanar (one interleaved chroma plane) or kPacked (one plane of four-byte groups)
    int swap;             // semi-planar: 1 = V first (NV21); packed: 1 = chroma first (UYVY)
};

YUV_HD bool format_traits(int format, Format* t) {
    switch (format) {
        case RELAX_YUVF_420P: *t = Format{1, 8, 0, 1, 1, kPlanar, 0}; return true;
        case RELAX_YUVF_422P: *t = Format{1, 8, 0, 1, 0, kPlanar, 0}; return true;
        case RELAX_YUVF_444P: *t = Format{1, 8, 0, 0, 0, kPlanar, 0}; return true;
        case RELAX_YUVF_NV12: *t = Format{1, 8, 0, 1, 1, kSemiPlanar, 0}; return true;
        case RELAX_YUVF_NV21: *t = Format{1, 8, 0, 1, 1, kSemiPlanar, 1}; return true;
        case RELAX_YUVF_YUYV422: *t = Format{1, 8, 0, 1, 0, kPacked, 0}; return true;
        case RELAX_YUVF_UYVY422: *t = Format{1, 8, 0, 1, 0, kPacked, 1}; return true;
        case RELAX_YUVF_411P: *t = Format{1, 8, 0, 2, 0, kPlanar, 0}; return true;
        case RELAX_YUVF_410P: *t = Format{1, 8, 0, 2, 2, kPlanar, 0}; return true;
        case RELAX_YUVF_420P10LE: *t = Format{2, 10, 0, 1, 1, kPlanar, 0}; return true;
        case RELAX_YUVF_422P10LE: *t = Format{2, 10, 0, 1, 0, kPlanar, 0}; return true;
        case RELAX_YUVF_444P10LE: *t = Format{2, 10, 0, 0, 0, kPlanar, 0}; return true;
        case RELAX_YUVF_420P12LE: *t = Format{2, 12, 0, 1, 1, kPlanar, 0}; return true;
        case RELAX_YUVF_422P12LE: *t = Format{2, 12, 0, 1, 0, kPlanar, 0}; return true;
        case RELAX_YUVF_444P12LE: *t = Format{2, 12, 0, 0, 0, kPlanar, 0}; return true;
        case RELAX_YUVF_P010LE: *t = Format{2, 10, 6, 1, 1, kSemiPlanar, 0}; return true;
        default: return false;
    }
}

struct Plan {
    int H, W;
    int cw, ch;           // chroma samples per row, chroma rows: ceil(W/2) x ceil(H/2) for 4:2:0, as ffmpeg lays raw frames out
    int hshift, vshift;   // pixel (r, c) takes chroma sample (r >> vshift, c >> hshift): replication, no interpolation
    int c_step;           // bytes from one chroma sample of a plane to the next: 1 planar, 2 for NV12's interleaved UV
    int64_t c_stride;     // bytes from one chroma row to the next: cw planar, 2*cw NV12
    int64_t u_off, v_off; // first U and first V byte, from the start of the frame
    int64_t frame_bytes;
    int64_t out_bytes;    // H*W*3: one output slot
    // what the RELAX_YUVF_* formats add (formats 0..3: 1, 8, 0, 255, kPlanar / kSemiPlanar, 0, 1, W, 0, 0 / 1)
    int sb, depth, shift; // Format's
    int mask;             // 2^depth - 1
    int packing;
    int y_off, y_step;    // first luma byte and bytes from one luma sample to the next: 0, sb - packed: 0 / 1 (UYVY), 2
    int64_t y_stride;     // bytes from one luma row to the next: W * sb - packed: 4 * cw
    int lu, lv;           // where U and V sit inside one lane's chroma segment on the 16-byte path: 0, 0 planar; 0 / sb semi-planar;
                          // packed: inside the four-byte group (1, 3 YUYV - 0, 2 UYVY)
};

// -> 0 and *p filled, or the number (1-based) of the offending argument: 1 format, 2 H, 3 W
YUV_HD int plan_ex(int format, int H, int W, Plan* p) {
    Format t;
    if (!format_traits(format, &t)) return 1;
    if (H < 1 || H > kMaxDim) return 2;
    if (W < 1 || W > kMaxDim) return 3;
    p->H = H;
    p->W = W;
    p->hshift = t.hshift;
    p->vshift = t.vshift;
    p->sb = t.sb, p->depth = t.depth, p->shift = t.shift, p->mask = (1 << t.depth) - 1, p->packing = t.packing;
    const int hr = (1 << t.hshift) - 1, vr = (1 << t.vshift) - 1;
    p->cw = (W + hr) >> t.hshift;
    p->ch = (H + vr) >> t.vshift;
    const int64_t y_bytes = static_cast<int64_t>(H) * W * t.sb;
    const int64_t c_bytes = static_cast<int64_t>(p->ch) * p->cw * t.sb;
    p->out_bytes = static_cast<int64_t>(H) * W * 3;
    if (t.packing == kPacked) {                                  // rows of cw groups Y0 U Y1 V (YUYV) / U Y0 V Y1 (UYVY)
        p->y_off = t.swap ? 1 : 0;
        p->y_step = 2;
        p->y_stride = 4 * static_cast<int64_t>(p->cw);
        p->c_step = 4;
        p->c_stride = p->y_stride;
        p->u_off = t.swap ? 0 : 1;
        p->v_off = p->u_off + 2;
        p->lu = static_cast<int>(p->u_off), p->lv = static_cast<int>(p->v_off);
        p->frame_bytes = p->y_stride * H;
        return 0;
    }
    p->y_off = 0;
    p->y_step = t.sb;
    p->y_stride = static_cast<int64_t>(W) * t.sb;
    if (t.packing == kSemiPlanar) {
        p->c_step = 2 * t.sb;
        p->c_stride = 2 * static_cast<int64_t>(p->cw) * t.sb;
        p->lu = t.swap ? t.sb : 0, p->lv = t.swap ? 0 : t.sb;
        p->u_off = y_bytes + p->lu;
        p->v_off = y_bytes + p->lv;
    } else {
        p->c_step = t.sb;
        p->c_stride = static_cast<int64_t>(p->cw) * t.sb;
        p->lu = p->lv = 0;
        p->u_off = y_bytes;
        p->v_off = y_bytes + c_bytes;
    }
    p->frame_bytes = y_bytes + 2 * c_bytes;
    return 0;
}

// the 8-bit layouts RELAX_YUV_420P..NV12 of relax_yuv_to_bgr: formats 0..3 of plan_ex, the same numbers
// -> 0 and *p filled, or the number (1-based) of the offending argument: 1 layout, 2 H, 3 W
YUV_HD int plan(int layout, int H, int W, Plan* p) {
    if (layout < RELAX_YUV_420P || layout > RELAX_YUV_NV12) return 1;
    return plan_ex(layout, H, W, p);
}

// byte offsets, from the start of the frame, of what pixel (r, c) reads
YUV_HD int64_t y_at(const Plan& p, int r, int c) { return static_cast<int64_t>(r) * p.W + c; }
YUV_HD int64_t u_at(const Plan& p, int r, int c) {
    return p.u_off + static_cast<int64_t>(r >> p.vshift) * p.c_stride + static_cast<int64_t>(c >> p.hshift) * p.c_step;
}
YUV_HD int64_t v_at(const Plan& p, int r, int c) {
    return p.v_off + static_cast<int64_t>(r >> p.vshift) * p.c_stride + static_cast<int64_t>(c >> p.hshift) * p.c_step;
}
// byte offset of pixel (r, c) inside its output slot
YUV_HD int64_t out_at(const Plan& p, int r, int c) { return (static_cast<int64_t>(r) * p.W + c) * 3; }

// an item may run iff its frame lies inside src and its slot inside out (written so that no sum can overflow)
YUV_HD bool item_in_range(const Plan& p, int64_t src_off, int64_t src_bytes, int64_t out_off, int64_t out_bytes) {
    return src_off >= 0 && p.frame_bytes <= src_bytes && src_off <= src_bytes - p.frame_bytes &&
           out_off >= 0 && p.out_bytes <= out_bytes && out_off <= out_bytes - p.out_bytes;
}

// Work units: one lane takes kLanePixels pixels of the rows that share a chroma row (2 rows for 4:2:0 / NV12, else 1).
constexpr int kLanePixels = 16;
YUV_HD int unit_cols(const Plan& p) { return (p.W + kLanePixels - 1) / kLanePixels; }
YUV_HD int unit_rows(const Plan& p) { return (p.H + p.vshift) >> p.vshift; }
YUV_HD int64_t units(const Plan& p) { return static_cast<int64_t>(unit_cols(p)) * unit_rows(p); }

// The 16-byte path: W a multiple of 16 and the frame's first byte and the slot's first byte at 16-byte-aligned ADDRESSES.  Then
// every Y segment, every 8-byte U / V segment (16-byte for 4:4:4 and NV12) and every 48-byte output segment of a lane is
// aligned to its access width: H*W, ch*cw and W*3 are all multiples of 16 (of 8: ch*cw for 4:2:0 / 4:2:2).
YUV_HD bool fast_path(const Plan& p, uint64_t src_addr, uint64_t out_addr) {
    return p.W % kLanePixels == 0 && src_addr % 16 == 0 && out_addr % 16 == 0;
}

// ---- colour -------------------------------------------------------------------------------------
// 16.16 fixed point: round(65536 * coefficient); limited range carries 255/219 on luma and 255/224 on chroma.
//   BT.601 (Kr 0.299, Kb 0.114) limited: swscale's table for untagged raw input.  Its full-range cgv is 46801 (the truncated
//   0.714136 * 65536 = 46801.6), kept as stated so that host, device and tests share one table.
//   BT.709 (Kr 0.2126, Kb 0.0722): crv = 2(1-Kr) = 1.5748, cbu = 2(1-Kb) = 1.8556, cgu = Kb*cbu/Kg = 0.187324,
//   cgv = Kr*crv/Kg = 0.468124 with Kg = 0.7152.
struct Coef {
    int cy, oy, crv, cbu, cgu, cgv;
};

YUV_HD bool coef(int matrix, int full_range, Coef* k) {
    if (matrix == RELAX_YUV_BT601) {
        if (full_range) *k = Coef{65536, 0, 91881, 116130, 22553, 46801};
        else *k = Coef{76309, 16, 104597, 132201, 25675, 53279};
        return true;
    }
    if (matrix == RELAX_YUV_BT709) {
        if (full_range) *k = Coef{65536, 0, 103206, 121609, 12276, 30679};
        else *k = Coef{76309, 16, 117489, 138438, 13975, 34925};
        return true;
    }
    return false;
}

// clip8(x >> 16), written as clamp-then-shift: min(max(x, 0), 2^24 - 1) >> 16 is the same value for every int x, and it keeps
// the compiler from forming gfx950's shift-and-saturate pack instruction (v_ashr_pk_u8_i32) out of two neighbouring channels:
// on the MI355X the words packed with it carried stale bits in their upper half (the first GPU run of the 16-byte path failed
// on exactly the bytes 2 and 3 of those words, the bytewise path passed).  The bit-equality cases of tests/test_gpu_yuv.py guard it.
YUV_HD int clip8_shift16(int x) {
    x = x < 0 ? 0 : (x > 0xffffff ? 0xffffff : x);
    return static_cast<int>(static_cast<unsigned>(x) >> 16);
}

// one pixel -> b, g, r.  |y| < 2^25 and every chroma term < 2^25: the sums stay far inside int32.
YUV_HD void pixel(const Coef& k, int Y, int U, int V, int* b, int* g, int* r) {
    const int y = k.cy * (Y - k.oy) + 32768;
    const int u = U - 128, v = V - 128;
    *r = clip8_shift16(y + k.crv * v);
    *g = clip8_shift16(y - k.cgu * u - k.cgv * v);
    *b = clip8_shift16(y + k.cbu * u);
}

// ---- what one lane touches ------------------------------------------------------------------------
struct Unit {
    int r0, c0;      // first row, first column
    int rows;        // 1 or 2 (2: the rows r0, r0 + 1 share the chroma row)
    int cols;        // 1..16 pixels
};

YUV_HD Unit unit_at(const Plan& p, int64_t unit) {
    const int ucols = unit_cols(p);
    Unit u;
    u.r0 = static_cast<int>(unit / ucols) << p.vshift;
    u.c0 = static_cast<int>(unit % ucols) * kLanePixels;
    u.rows = (p.vshift && u.r0 + 1 < p.H) ? 2 : 1;
    u.cols = p.W - u.c0 < kLanePixels ? p.W - u.c0 : kLanePixels;
    return u;
}

// the accesses of a lane on the 16-byte path (fast_path() holds, so cols == 16): offsets from the frame's / the slot's start
struct FastUnit {
    int rows;
    int64_t y[2];      // 16 bytes each
    int64_t u, v;      // c_bytes each; NV12 reads its 16 interleaved bytes at u alone (v = u + 1 is not an access)
    int c_bytes;       // 8 for 4:2:0 / 4:2:2, 16 for 4:4:4 and NV12
    int64_t o[2];      // 48 bytes each: three 16-byte stores
};

YUV_HD FastUnit fast_unit(const Plan& p, int64_t unit) {
    const Unit u = unit_at(p, unit);
    FastUnit f;
    f.rows = u.rows;
    f.y[0] = y_at(p, u.r0, u.c0);
    f.y[1] = y_at(p, u.r0 + u.rows - 1, u.c0);
    f.u = u_at(p, u.r0, u.c0);
    f.v = v_at(p, u.r0, u.c0);
    f.c_bytes = (p.c_step == 2 || p.hshift == 0) ? 16 : 8;
    f.o[0] = out_at(p, u.r0, u.c0);
    f.o[1] = out_at(p, u.r0 + u.rows - 1, u.c0);
    return f;
}

// the bytewise path of one lane: any W, any base; every index below its bound (r < H, c < W)
YUV_HD void unit_bytewise(const Plan& p, const Coef& k, const uint8_t* f, uint8_t* o, int64_t unit) {
    const Unit u = unit_at(p, unit);
    for (int r = u.r0; r < u.r0 + u.rows; ++r) {
        for (int c = u.c0; c < u.c0 + u.cols; ++c) {
            int b, g, rr;
            pixel(k, f[y_at(p, r, c)], f[u_at(p, r, c)], f[v_at(p, r, c)], &b, &g, &rr);
            uint8_t* q = o + out_at(p, r, c);
            q[0] = static_cast<uint8_t>(b);
            q[1] = static_cast<uint8_t>(g);
            q[2] = static_cast<uint8_t>(rr);
        }
    }
}

// ---- the RELAX_YUVF_* formats: any depth up to 12, 1 / 2 / 4 rows per unit ------------------------------------------------------
// one formula for every depth, s = depth - 8: at s = 0 it is pixel() bit for bit, in the same clamp-then-shift form (see
// clip8_shift16).  depth <= 12: |y| < 2^29 and every chroma term < 2^29, the sums stay inside int32.
YUV_HD int clip8_shift_ex(int x, int s) {
    const int top = (1 << (24 + s)) - 1;
    x = x < 0 ? 0 : (x > top ? top : x);
    return static_cast<int>(static_cast<unsigned>(x) >> (16 + s));
}

YUV_HD void pixel_ex(const Coef& k, int s, int Y, int U, int V, int* b, int* g, int* r) {
    const int y = k.cy * (Y - (k.oy << s)) + (1 << (15 + s));
    const int u = U - (128 << s), v = V - (128 << s);
    *r = clip8_shift_ex(y + k.crv * v, s);
    *g = clip8_shift_ex(y - k.cgu * u - k.cgv * v, s);
    *b = clip8_shift_ex(y + k.cbu * u, s);
}

// byte offsets of what pixel (r, c) reads: u_at / v_at above hold for every format (a packed row is its own chroma row)
YUV_HD int64_t y_at_ex(const Plan& p, int r, int c) { return p.y_off + static_cast<int64_t>(r) * p.y_stride + static_cast<int64_t>(c) * p.y_step; }

// the sample whose first byte is f[off]
YUV_HD int sample_at(const Plan& p, const uint8_t* f, int64_t off) {
    const int w = p.sb == 1 ? f[off] : (f[off] | (f[off + 1] << 8));
    return (w >> p.shift) & p.mask;
}

YUV_HD int unit_rows_ex(const Plan& p) { return (p.H + (1 << p.vshift) - 1) >> p.vshift; }
YUV_HD int64_t units_ex(const Plan& p) { return static_cast<int64_t>(unit_cols(p)) * unit_rows_ex(p); }

YUV_HD Unit unit_at_ex(const Plan& p, int64_t unit) {
    const int ucols = unit_cols(p);
    Unit u;
    u.r0 = static_cast<int>(unit / ucols) << p.vshift;
    u.c0 = static_cast<int>(unit % ucols) * kLanePixels;
    u.rows = p.H - u.r0 < (1 << p.vshift) ? p.H - u.r0 : (1 << p.vshift);
    u.cols = p.W - u.c0 < kLanePixels ? p.W - u.c0 : kLanePixels;
    return u;
}

// one pixel of the bytewise path: any W, any base; r < H, c < W
YUV_HD void pixel_bytewise_ex(const Plan& p, const Coef& k, const uint8_t* f, int r, int c, int* b, int* g, int* rr) {
    pixel_ex(k, p.depth - 8, sample_at(p, f, y_at_ex(p, r, c)), sample_at(p, f, u_at(p, r, c)), sample_at(p, f, v_at(p, r, c)), b, g, rr);
}

YUV_HD void unit_bytewise_ex(const Plan& p, const Coef& k, const uint8_t* f, uint8_t* o, int64_t unit) {
    const Unit u = unit_at_ex(p, unit);
    for (int r = u.r0; r < u.r0 + u.rows; ++r) {
        for (int c = u.c0; c < u.c0 + u.cols; ++c) {
            int b, g, rr;
            pixel_bytewise_ex(p, k, f, r, c, &b, &g, &rr);
            uint8_t* q = o + out_at(p, r, c);
            q[0] = static_cast<uint8_t>(b);
            q[1] = static_cast<uint8_t>(g);
            q[2] = static_cast<uint8_t>(rr);
        }
    }
}

// The 16-byte path of the RELAX_YUVF_* formats, under fast_path()'s condition.  With W a multiple of 16 and an aligned frame
// every plane starts at a multiple of 16 (4:1:x chroma planes: of 4), a lane's luma segment is 16 * y_step bytes and its chroma
// segment (16 >> hshift) * c_step bytes, each aligned to its access width.
struct FastUnitEx {
    int rows;          // 1, 2 or 4
    int64_t y[4];      // y_bytes each, as 16-byte loads; rows beyond `rows` repeat the last one and are no access
    int y_bytes;       // 16, or 32: 16-bit luma and packed rows (which hold their chroma)
    int c_planes;      // 2 planar, 1 semi-planar (one segment at c[0] holds both), 0 packed
    int64_t c[2];      // c_bytes each, as accesses of c_width: U, V - semi-planar: the interleaved segment
    int c_bytes;       // 4 (4:1:1 / 4:1:0), 8, 16 or 32
    int c_width;       // 4, 8 or 16
    int64_t o[4];      // 48 bytes each: three 16-byte stores
};

YUV_HD FastUnitEx fast_unit_ex(const Plan& p, int64_t unit) {
    const Unit u = unit_at_ex(p, unit);
    FastUnitEx f;
    f.rows = u.rows;
    for (int j = 0; j < 4; ++j) {
        const int r = u.r0 + (j < u.rows ? j : u.rows - 1);
        f.y[j] = y_at_ex(p, r, u.c0) - p.y_off;
        f.o[j] = out_at(p, r, u.c0);
    }
    f.y_bytes = kLanePixels * p.y_step;
    f.c_planes = p.packing == kPacked ? 0 : (p.packing == kSemiPlanar ? 1 : 2);
    f.c[0] = u_at(p, u.r0, u.c0) - p.lu;
    f.c[1] = v_at(p, u.r0, u.c0) - p.lv;
    f.c_bytes = f.c_planes ? (kLanePixels >> p.hshift) * p.c_step : 0;
    f.c_width = f.c_bytes < 16 ? f.c_bytes : 16;
    return f;
}

// What the kernels are specialised on: sample bytes, packing, hshift, vshift.  A lane's segments live in words (registers on the
// device): lw the luma row (kYWords), cu and cv the chroma segments (kCWords; semi-planar: both the one interleaved segment;
// packed: both the luma row).  Shift, mask and the place of U and V inside a segment (Plan's y_off, lu, lv) are uniform values.
template <int SB, int PACK, int HS, int VS>
struct Kind {
    static constexpr int kRows = 1 << VS;
    static constexpr int kYStep = PACK == kPacked ? 2 : SB;
    static constexpr int kCStep = PACK == kPacked ? 4 : (PACK == kSemiPlanar ? 2 * SB : SB);
    static constexpr int kYWords = kLanePixels * kYStep / 4;
    static constexpr int kCBytes = PACK == kPacked ? 0 : (kLanePixels >> HS) * kCStep;
    static constexpr int kCWords = PACK == kPacked ? kYWords : kCBytes / 4;
    static constexpr int kCPlanes = PACK == kPacked ? 0 : (PACK == kSemiPlanar ? 1 : 2);
    YUV_HD static bool matches(const Plan& p) { return p.sb == SB && p.packing == PACK && p.hshift == HS && p.vshift == VS; }
    // the sample at byte `at + add` of a segment: `at` a constant once the loops are unrolled, (at & 3) + add < 4
    YUV_HD static int sample(const Plan& p, const uint32_t* w, int at, int add) {
        const uint32_t x = w[at >> 2] >> (((at & 3) + add) * 8);
        if (SB == 1) return static_cast<int>(x & 255u);
        return static_cast<int>(((x & 0xffffu) >> p.shift) & static_cast<uint32_t>(p.mask));
    }
    // pixel px (0..15) of a lane's row
    YUV_HD static void pixel(const Plan& p, const Coef& k, const uint32_t* lw, const uint32_t* cu, const uint32_t* cv, int px, int* b,
                             int* g, int* r) {
        const int Y = sample(p, lw, px * kYStep, p.y_off);
        const int U = sample(p, cu, (px >> HS) * kCStep, p.lu);
        const int V = sample(p, cv, (px >> HS) * kCStep, p.lv);
        pixel_ex(k, p.depth - 8, Y, U, V, b, g, r);
    }
};

// The one place that maps a plan to its kind: F<SB, PACK, HS, VS>::get() of the plan's kind (a kernel, a host lane, ...).  The eight
// kinds of the formats from NV21 on (NV12 shares NV21's); with kWithLayouts also the three 8-bit planar kinds of formats 0..2, which
// the device never launches (relax_yuv_to_bgr's kernel takes those) - without it they give a null result.
template <template <int, int, int, int> class F, bool kWithLayouts>
inline auto for_kind(const Plan& p) -> decltype(F<1, kPacked, 1, 0>::get()) {
    if (p.packing == kPacked) return F<1, kPacked, 1, 0>::get();
    if (p.packing == kSemiPlanar) return p.sb == 2 ? F<2, kSemiPlanar, 1, 1>::get() : F<1, kSemiPlanar, 1, 1>::get();
    if (p.sb == 2) {
        if (p.hshift == 0) return F<2, kPlanar, 0, 0>::get();
        return p.vshift ? F<2, kPlanar, 1, 1>::get() : F<2, kPlanar, 1, 0>::get();
    }
    if (p.hshift == 2) return p.vshift == 2 ? F<1, kPlanar, 2, 2>::get() : F<1, kPlanar, 2, 0>::get();
    if constexpr (kWithLayouts) {
        if (p.hshift == 0) return F<1, kPlanar, 0, 0>::get();
        return p.vshift ? F<1, kPlanar, 1, 1>::get() : F<1, kPlanar, 1, 0>::get();
    } else {
        return nullptr;
    }
}

}  // namespace yuv
