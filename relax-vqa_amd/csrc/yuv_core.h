// Raw 8-bit YUV frames -> BGR: frame layout, per-item bounds and the integer colour arithmetic of relax_yuv_to_bgr
// (include/relax_hip.h), with no HIP in it.  yuv.hip compiles it for the device; yuv_host.cpp compiles the same text for the
// host (the stand-alone sanitizer program behind `make sanitize_yuv`), so the offsets a kernel lane uses are the offsets the
// CPU test walks.
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

struct Plan {
    int H, W;
    int cw, ch;           // chroma samples per row, chroma rows: ceil(W/2) x ceil(H/2) for 4:2:0, as ffmpeg lays raw frames out
    int hshift, vshift;   // pixel (r, c) takes chroma sample (r >> vshift, c >> hshift): replication, no interpolation
    int c_step;           // bytes from one chroma sample of a plane to the next: 1 planar, 2 for NV12's interleaved UV
    int64_t c_stride;     // bytes from one chroma row to the next: cw planar, 2*cw NV12
    int64_t u_off, v_off; // first U and first V byte, from the start of the frame
    int64_t frame_bytes;
    int64_t out_bytes;    // H*W*3: one output slot
};

// -> 0 and *p filled, or the number (1-based) of the offending argument: 1 layout, 2 H, 3 W
YUV_HD int plan(int layout, int H, int W, Plan* p) {
    if (layout < RELAX_YUV_420P || layout > RELAX_YUV_NV12) return 1;
    if (H < 1 || H > kMaxDim) return 2;
    if (W < 1 || W > kMaxDim) return 3;
    p->H = H;
    p->W = W;
    p->hshift = layout == RELAX_YUV_444P ? 0 : 1;
    p->vshift = (layout == RELAX_YUV_420P || layout == RELAX_YUV_NV12) ? 1 : 0;
    p->cw = (W + p->hshift) >> p->hshift;
    p->ch = (H + p->vshift) >> p->vshift;
    const int64_t y_bytes = static_cast<int64_t>(H) * W;
    const int64_t c_bytes = static_cast<int64_t>(p->ch) * p->cw;
    p->u_off = y_bytes;
    if (layout == RELAX_YUV_NV12) {
        p->c_step = 2;
        p->c_stride = 2 * static_cast<int64_t>(p->cw);
        p->v_off = y_bytes + 1;
    } else {
        p->c_step = 1;
        p->c_stride = p->cw;
        p->v_off = y_bytes + c_bytes;
    }
    p->frame_bytes = y_bytes + 2 * c_bytes;
    p->out_bytes = y_bytes * 3;
    return 0;
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

}  // namespace yuv
