// greyscale_core.h on the host: every lane of relax_greyscale_scan's and relax_yuv_greyscale_scan's grids played in turn - the
// same units, the same accesses (a memcpy of the access width at the access offset), the same arithmetic, the records merged by
// maximum as the device's atomics merge them.  Built two ways:
//   librelax_greyscale_host.so   grey_host_scan_bgr / grey_host_scan_yuv, which tests/test_greyscale_cpu.py holds against the numpy
//                                statement of the rule;
//   greyscale_san                with -DGREYSCALE_MAIN, its own main under AddressSanitizer + UBSan (`make greyscale_san`): the
//                                grids run against heap buffers of exactly the stated sizes, so an access outside a frame is a
//                                sanitizer report, and the records are compared with the rule written pixel by pixel.
// `align` stands for the address of the buffer's first byte modulo 16: the host's own addresses play no part.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "greyscale_core.h"

namespace {

void merge(int32_t* rec, const grey::Acc& a) {
    int32_t m[6];
    grey::finish(a, m);
    for (int q = 0; q < 6; ++q) rec[q] = m[q] > rec[q] ? m[q] : rec[q];
}

void bgr_lane(const uint8_t* f, uint64_t addr, int64_t npix, int64_t block, int lane, int32_t* rec) {
    const int64_t nunits = grey::units(npix);
    grey::Acc a;
    grey::init(&a);
    for (int j = 0; j < grey::kLaneUnits; ++j) {
        const int64_t unit = grey::unit_of(block, lane, j);
        if (grey::fast_path(addr) && grey::unit_is_full(npix, unit)) {
            uint32_t w[12];
            for (int i = 0; i < 3; ++i) std::memcpy(w + 4 * i, f + unit * (grey::kLanePixels * 3) + 16 * i, 16);
            grey::unit_words(&a, w);
        } else if (unit < nunits) {
            grey::unit_bytewise(&a, f, npix, unit);
        }
    }
    merge(rec, a);
}

void yuv_lane(const yuv::Plan& p, const yuv::Coef& k, int layout, const uint8_t* f, uint64_t addr, int64_t block, int lane,
              int32_t* rec) {
    const int64_t nunits = yuv::units(p);
    grey::Acc a;
    grey::init(&a);
    for (int j = 0; j < grey::kLaneUnits; ++j) {
        const int64_t unit = grey::unit_of(block, lane, j);
        if (unit >= nunits) continue;
        if (!grey::yuv_fast_path(p, addr)) {
            grey::yuv_unit_bytewise(&a, p, k, f, unit);
            continue;
        }
        const yuv::FastUnit u = yuv::fast_unit(p, unit);
        uint32_t cu[4], cv[4], in[4], in2[4], y[4];
        if (layout == RELAX_YUV_NV12) {
            std::memcpy(in, f + u.u, 16);
            grey::split_nv12(in, cu, cv);
        } else if (u.c_bytes == 16) {
            std::memcpy(cu, f + u.u, 16);
            std::memcpy(cv, f + u.v, 16);
        } else {
            std::memcpy(in, f + u.u, 8);
            std::memcpy(in2, f + u.v, 8);
            grey::widen8(in, cu);
            grey::widen8(in2, cv);
        }
        for (int r = 0; r < u.rows; ++r) {
            std::memcpy(y, f + u.y[r], 16);
            grey::yuv_row16(&a, k, y, cu, cv);
        }
    }
    merge(rec, a);
}

}  // namespace

extern "C" int grey_host_scan_bgr(const uint8_t* frames, int64_t frame_stride, int N, int H, int W, int align, int32_t* out) {
    if (grey::check_size(H, W) != 0 || N < 0 || (N > 0 && (!frames || !out))) return RELAX_ERR_INVALID;
    const int64_t npix = grey::pixels(H, W);
    if (N > 1 && frame_stride < npix * 3) return RELAX_ERR_INVALID;
    for (int n = 0; n < N; ++n) {
        int32_t* rec = out + static_cast<int64_t>(n) * grey::kRecordWords;
        std::memset(rec, 0, sizeof(int32_t) * grey::kRecordWords);
        const int64_t off = static_cast<int64_t>(n) * frame_stride;
        for (int64_t b = 0; b < grey::blocks(grey::units(npix)); ++b)
            for (int lane = 0; lane < grey::kBlock; ++lane)
                bgr_lane(frames + off, static_cast<uint64_t>(align) + static_cast<uint64_t>(off), npix, b, lane, rec);
    }
    return RELAX_OK;
}

extern "C" int grey_host_scan_yuv(const uint8_t* src, int64_t src_bytes, const int64_t* offsets, int N, int layout, int H, int W,
                                  int matrix, int full_range, int align, int32_t* out) {
    yuv::Plan p;
    yuv::Coef k;
    if (yuv::plan(layout, H, W, &p) != 0 || !yuv::coef(matrix, full_range, &k) || (full_range != 0 && full_range != 1)) return RELAX_ERR_INVALID;
    if (N < 0 || src_bytes < 0 || (N > 0 && (!offsets || !out || !src))) return RELAX_ERR_INVALID;
    for (int n = 0; n < N; ++n) {
        int32_t* rec = out + static_cast<int64_t>(n) * grey::kRecordWords;
        std::memset(rec, 0, sizeof(int32_t) * grey::kRecordWords);
        if (!grey::yuv_frame_in_range(p, offsets[n], src_bytes)) {
            rec[grey::kStatusWord] = RELAX_YUV_OUT_OF_RANGE;
            continue;
        }
        for (int64_t b = 0; b < grey::blocks(yuv::units(p)); ++b)
            for (int lane = 0; lane < grey::kBlock; ++lane)
                yuv_lane(p, k, layout, src + offsets[n], static_cast<uint64_t>(align) + static_cast<uint64_t>(offsets[n]), b, lane, rec);
    }
    return RELAX_OK;
}

#ifdef GREYSCALE_MAIN
namespace {

int failures = 0;

void fail(const char* what, int H, int W, long long a = 0, long long b = 0) {
    std::printf("MISMATCH %s: H %d W %d (%lld vs %lld)\n", what, H, W, a, b);
    ++failures;
}

uint32_t rng_state = 2463534242u;
uint8_t next_byte() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return static_cast<uint8_t>(rng_state >> 24);
}

// the rule pixel by pixel, on uint8 as the reference's numpy views compute it
void rule(const uint8_t* bgr, int64_t npix, int32_t* rec) {
    std::memset(rec, 0, sizeof(int32_t) * grey::kRecordWords);
    for (int64_t i = 0; i < npix; ++i) {
        const uint8_t b = bgr[3 * i], g = bgr[3 * i + 1], r = bgr[3 * i + 2];
        const int32_t v[6] = {static_cast<uint8_t>(b - g), static_cast<uint8_t>(b - r), static_cast<uint8_t>(g - r),
                              b > g ? b - g : g - b, b > r ? b - r : r - b, g > r ? g - r : r - g};
        for (int q = 0; q < 6; ++q) rec[q] = v[q] > rec[q] ? v[q] : rec[q];
    }
}

bool same(const int32_t* a, const int32_t* b) { return std::memcmp(a, b, sizeof(int32_t) * grey::kRecordWords) == 0; }

// three frames in strided slots of a buffer that ends with the last frame; near-grey content so that both rules see small and
// wrapped values; every alignment class
void bgr_geometry(int H, int W, int mode) {
    const int64_t npix = grey::pixels(H, W), slot = npix * 3, stride = slot + 7;
    const int frames = 3;
    std::vector<uint8_t> buf(static_cast<size_t>((frames - 1) * stride + slot));
    for (int n = 0; n < frames; ++n)
        for (int64_t i = 0; i < npix; ++i) {
            uint8_t* q = buf.data() + n * stride + 3 * i;
            const uint8_t v = next_byte();
            if (mode == 0) q[0] = next_byte(), q[1] = next_byte(), q[2] = next_byte();
            else q[0] = static_cast<uint8_t>(v + next_byte() % 4), q[1] = static_cast<uint8_t>(v + next_byte() % 3), q[2] = v;
        }
    std::vector<int32_t> want(frames * grey::kRecordWords), got(frames * grey::kRecordWords, 0x7f7f7f7f);
    for (int n = 0; n < frames; ++n) rule(buf.data() + n * stride, npix, want.data() + n * grey::kRecordWords);
    for (int align = 0; align < 16; align += 5) {
        if (grey_host_scan_bgr(buf.data(), stride, frames, H, W, align, got.data()) != RELAX_OK) fail("bgr scan refused", H, W);
        for (int n = 0; n < frames; ++n)
            if (!same(got.data() + n * grey::kRecordWords, want.data() + n * grey::kRecordWords))
                fail("bgr record differs from the rule", H, W, n, align);
    }
}

// the plane-by-plane conversion of yuv_host.cpp, then the rule
void yuv_reference(int layout, int H, int W, const yuv::Coef& k, const uint8_t* f, int32_t* rec) {
    const int sub_w = layout != RELAX_YUV_444P, sub_h = layout == RELAX_YUV_420P || layout == RELAX_YUV_NV12;
    const int cw = sub_w ? (W + 1) / 2 : W, ch = sub_h ? (H + 1) / 2 : H;
    const uint8_t* up = f + static_cast<size_t>(H) * W;
    const uint8_t* vp = up + static_cast<size_t>(ch) * cw;
    std::vector<uint8_t> bgr(static_cast<size_t>(H) * W * 3);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            const size_t ci = static_cast<size_t>(sub_h ? r / 2 : r) * cw + (sub_w ? c / 2 : c);
            const int U = layout == RELAX_YUV_NV12 ? up[ci * 2] : up[ci], V = layout == RELAX_YUV_NV12 ? up[ci * 2 + 1] : vp[ci];
            int b, g, rr;
            yuv::pixel(k, f[static_cast<size_t>(r) * W + c], U, V, &b, &g, &rr);
            uint8_t* q = bgr.data() + (static_cast<size_t>(r) * W + c) * 3;
            q[0] = static_cast<uint8_t>(b), q[1] = static_cast<uint8_t>(g), q[2] = static_cast<uint8_t>(rr);
        }
    rule(bgr.data(), static_cast<int64_t>(H) * W, rec);
}

void yuv_geometry(int layout, int H, int W, int matrix, int full) {
    yuv::Plan p;
    yuv::Coef k;
    if (yuv::plan(layout, H, W, &p) != 0 || !yuv::coef(matrix, full, &k)) return fail("plan refused", H, W, layout);
    const int frames = 3;
    std::vector<uint8_t> src(static_cast<size_t>(p.frame_bytes) * frames);   // exactly three frames: a byte beyond is a report
    for (size_t i = 0; i < src.size(); ++i) {
        const bool chroma = static_cast<int64_t>(i % p.frame_bytes) >= p.u_off;
        src[i] = chroma ? static_cast<uint8_t>(126 + next_byte() % 5) : next_byte();      // near-neutral chroma: both sides of the threshold
    }
    const int64_t sb = static_cast<int64_t>(src.size());
    const int64_t offsets[6] = {2 * p.frame_bytes, 0, p.frame_bytes, sb - p.frame_bytes + 1, -1, sb};
    std::vector<int32_t> got(6 * grey::kRecordWords, 0x7f7f7f7f), want(grey::kRecordWords);
    for (int align = 0; align < 2; ++align) {
        if (grey_host_scan_yuv(src.data(), sb, offsets, 6, layout, H, W, matrix, full, align, got.data()) != RELAX_OK)
            fail("yuv scan refused", H, W, layout);
        for (int n = 0; n < 3; ++n) {
            yuv_reference(layout, H, W, k, src.data() + offsets[n], want.data());
            if (!same(got.data() + n * grey::kRecordWords, want.data())) fail("yuv record differs from convert-then-rule", H, W, layout, n);
        }
        for (int n = 3; n < 6; ++n) {
            std::memset(want.data(), 0, sizeof(int32_t) * grey::kRecordWords);
            want[grey::kStatusWord] = RELAX_YUV_OUT_OF_RANGE;
            if (!same(got.data() + n * grey::kRecordWords, want.data())) fail("out-of-range frame's record", H, W, layout, n);
        }
    }
}

}  // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {2, 16}, {6, 48}, {7, 50}, {3, 17}, {5, 15}, {2, 2}, {18, 34}, {131, 97}, {32, 64}, {67, 256}};   // H, W
    for (const auto& s : sizes) {
        for (int mode = 0; mode < 2; ++mode) bgr_geometry(s[0], s[1], mode);
        for (int layout = RELAX_YUV_420P; layout <= RELAX_YUV_NV12; ++layout)
            for (int m = 0; m < 4; ++m) {
                if (m && s[0] * s[1] > 64 * 32) continue;
                yuv_geometry(layout, s[0], s[1], m >> 1, m & 1);
            }
        std::printf("geometry %d %d : units %lld blocks %lld\n", s[0], s[1], static_cast<long long>(grey::units(grey::pixels(s[0], s[1]))),
                    static_cast<long long>(grey::blocks(grey::units(grey::pixels(s[0], s[1])))));
    }
    // every pair of byte values through the extremes: the wrapped and the absolute value of one difference
    for (int x = 0; x < 256; ++x)
        for (int y = 0; y < 256; ++y) {
            grey::Acc a;
            grey::init(&a);
            grey::add(&a, x, y, y);
            int32_t m[6];
            grey::finish(a, m);
            if (m[0] != ((x - y) & 255) || m[3] != (x > y ? x - y : y - x) || m[2] != 0 || m[5] != 0) fail("one pixel", x, y, m[0], m[3]);
        }
    int32_t rec[grey::kRecordWords];
    uint8_t px[3] = {1, 2, 3};
    if (grey_host_scan_bgr(px, 3, 1, 0, 1, 0, rec) == RELAX_OK || grey_host_scan_bgr(px, 3, 1, 1, yuv::kMaxDim + 1, 0, rec) == RELAX_OK ||
        grey_host_scan_bgr(px, 3, -1, 1, 1, 0, rec) == RELAX_OK || grey_host_scan_bgr(nullptr, 3, 1, 1, 1, 0, rec) == RELAX_OK ||
        grey_host_scan_bgr(px, 2, 2, 1, 1, 0, rec) == RELAX_OK)
        fail("a refusal", 0, 0);
    std::printf(failures ? "FAILED %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
#endif
