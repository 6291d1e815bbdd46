// yuv_core.h on the host, with its own main: the stand-alone program behind `make sanitize_yuv` (AddressSanitizer + UBSan,
// CPU only; tests/test_yuv_cpu.py runs it).  For every layout and a list of geometries it plays every lane of
// relax_yuv_to_bgr's grid - the bytewise path, and the 16-byte path where it applies - against heap buffers of exactly
// the sizes the C-ABI states, so an access outside a frame or a slot is a sanitizer report; it checks the bytes against a
// conversion written plane by plane, that every output byte is written exactly once, and the out-of-range item rule.
// Prints one line per geometry (the test compares them with the Python arithmetic) and exits non-zero on any mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "yuv_core.h"

namespace {

int failures = 0;

void fail(const char* what, int layout, int H, int W, long long a = 0, long long b = 0) {
    std::printf("MISMATCH %s: layout %d H %d W %d (%lld vs %lld)\n", what, layout, H, W, a, b);
    ++failures;
}

uint32_t rng_state = 12345;
uint8_t next_byte() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return static_cast<uint8_t>(rng_state >> 24);
}

// the conversion written plane by plane, without yuv_core.h's offset functions
void reference(int layout, int H, int W, const yuv::Coef& k, const uint8_t* f, uint8_t* o) {
    const int sub_w = layout != RELAX_YUV_444P, sub_h = layout == RELAX_YUV_420P || layout == RELAX_YUV_NV12;
    const int cw = sub_w ? (W + 1) / 2 : W, ch = sub_h ? (H + 1) / 2 : H;
    const uint8_t* yp = f;
    const uint8_t* up = f + static_cast<size_t>(H) * W;
    const uint8_t* vp = up + static_cast<size_t>(ch) * cw;
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            const int cr = sub_h ? r / 2 : r, cc = sub_w ? c / 2 : c;
            int U, V;
            if (layout == RELAX_YUV_NV12) {
                U = up[(static_cast<size_t>(cr) * cw + cc) * 2];
                V = up[(static_cast<size_t>(cr) * cw + cc) * 2 + 1];
            } else {
                U = up[static_cast<size_t>(cr) * cw + cc];
                V = vp[static_cast<size_t>(cr) * cw + cc];
            }
            int b, g, rr;
            yuv::pixel(k, yp[static_cast<size_t>(r) * W + c], U, V, &b, &g, &rr);
            uint8_t* q = o + (static_cast<size_t>(r) * W + c) * 3;
            q[0] = static_cast<uint8_t>(b), q[1] = static_cast<uint8_t>(g), q[2] = static_cast<uint8_t>(rr);
        }
}

// a lane of the 16-byte path: the same accesses (memcpy of the access width at the access offset), scalar arithmetic
void fast_lane(const yuv::Plan& p, int layout, const yuv::Coef& k, const uint8_t* f, uint8_t* o, int64_t unit,
               std::vector<uint8_t>& hits) {
    const yuv::FastUnit a = yuv::fast_unit(p, unit);
    uint8_t y[2][16], cu[16], cv[16], raw[32];
    if (a.y[0] % 16 || a.y[1] % 16 || a.u % a.c_bytes || (layout != RELAX_YUV_NV12 && a.v % a.c_bytes) || a.o[0] % 16 || a.o[1] % 16)
        fail("misaligned fast access", layout, p.H, p.W, a.u, a.v);
    if (layout == RELAX_YUV_NV12) {
        std::memcpy(raw, f + a.u, 16);
        for (int i = 0; i < 16; ++i) cu[i] = raw[(i / 2) * 2], cv[i] = raw[(i / 2) * 2 + 1];
    } else if (a.c_bytes == 16) {
        std::memcpy(cu, f + a.u, 16);
        std::memcpy(cv, f + a.v, 16);
    } else {
        std::memcpy(raw, f + a.u, 8);
        std::memcpy(raw + 8, f + a.v, 8);
        for (int i = 0; i < 16; ++i) cu[i] = raw[i / 2], cv[i] = raw[8 + i / 2];
    }
    for (int j = 0; j < a.rows; ++j) std::memcpy(y[j], f + a.y[j], 16);
    for (int j = 0; j < a.rows; ++j) {
        uint8_t px[48];
        for (int i = 0; i < 16; ++i) {
            int b, g, r;
            yuv::pixel(k, y[j][i], cu[i], cv[i], &b, &g, &r);
            px[3 * i] = static_cast<uint8_t>(b), px[3 * i + 1] = static_cast<uint8_t>(g), px[3 * i + 2] = static_cast<uint8_t>(r);
        }
        std::memcpy(o + a.o[j], px, 48);
        for (int i = 0; i < 48; ++i) ++hits[static_cast<size_t>(a.o[j]) + i];
    }
}

void geometry(int layout, int H, int W, int matrix, int full) {
    yuv::Plan p;
    yuv::Coef k;
    if (yuv::plan(layout, H, W, &p) != 0 || !yuv::coef(matrix, full, &k)) return fail("plan refused", layout, H, W);
    std::printf("plan %d %d %d : frame_bytes %lld u_off %lld v_off %lld cw %d ch %d c_stride %lld c_step %d units %lld fast %d\n", layout, H, W,
                static_cast<long long>(p.frame_bytes), static_cast<long long>(p.u_off), static_cast<long long>(p.v_off), p.cw,
                p.ch, static_cast<long long>(p.c_stride), p.c_step, static_cast<long long>(yuv::units(p)),
                static_cast<int>(yuv::fast_path(p, 0, 0)));
    const int frames = 3;
    // exactly frames * frame_bytes and frames * H*W*3 bytes on the heap: one byte beyond either is a sanitizer report
    std::vector<uint8_t> src(static_cast<size_t>(p.frame_bytes) * frames);
    for (auto& b : src) b = next_byte();
    std::vector<uint8_t> out(static_cast<size_t>(p.out_bytes) * frames), want(out.size()), fast(out.size());
    for (int n = 0; n < frames; ++n) {
        const int64_t so = n * p.frame_bytes, oo = (frames - 1 - n) * p.out_bytes;      // slots in reverse order
        if (!yuv::item_in_range(p, so, static_cast<int64_t>(src.size()), oo, static_cast<int64_t>(out.size())))
            fail("an item inside its buffers was refused", layout, H, W, so, oo);
        reference(layout, H, W, k, src.data() + so, want.data() + oo);
        for (int64_t u = 0; u < yuv::units(p); ++u) yuv::unit_bytewise(p, k, src.data() + so, out.data() + oo, u);
        if (yuv::fast_path(p, 0, 0)) {
            std::vector<uint8_t> hits(static_cast<size_t>(p.out_bytes), 0);
            for (int64_t u = 0; u < yuv::units(p); ++u) fast_lane(p, layout, k, src.data() + so, fast.data() + oo, u, hits);
            for (size_t i = 0; i < hits.size(); ++i)
                if (hits[i] != 1) {
                    fail("an output byte written other than once", layout, H, W, static_cast<long long>(i), hits[i]);
                    break;
                }
        }
    }
    if (out != want) fail("bytewise path differs from the plane-by-plane conversion", layout, H, W);
    if (yuv::fast_path(p, 0, 0) && fast != want) fail("16-byte path differs from the plane-by-plane conversion", layout, H, W);
    // the out-of-range rule, at the edges and at values whose sums would overflow
    const int64_t sb = static_cast<int64_t>(src.size()), ob = static_cast<int64_t>(out.size());
    const int64_t big = std::numeric_limits<int64_t>::max(), small = std::numeric_limits<int64_t>::min();
    const int64_t bad_src[] = {-1, sb - p.frame_bytes + 1, sb, big, small};
    const int64_t bad_out[] = {-1, ob - p.out_bytes + 1, ob, big, small};
    for (int64_t s : bad_src)
        if (yuv::item_in_range(p, s, sb, 0, ob)) fail("source offset accepted", layout, H, W, s, sb);
    for (int64_t o : bad_out)
        if (yuv::item_in_range(p, 0, sb, o, ob)) fail("output offset accepted", layout, H, W, o, ob);
    if (!yuv::item_in_range(p, sb - p.frame_bytes, sb, ob - p.out_bytes, ob)) fail("last slot refused", layout, H, W);
    if (yuv::item_in_range(p, 0, p.frame_bytes - 1, 0, ob) || yuv::item_in_range(p, 0, sb, 0, p.out_bytes - 1) ||
        yuv::item_in_range(p, 0, 0, 0, 0))
        fail("buffer shorter than one frame accepted", layout, H, W);
}

}  // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {2, 2}, {3, 5}, {2, 16}, {18, 34}, {131, 97}, {32, 64}, {5, 16}, {7, 48}, {16, 17}, {1, 32}, {33, 15}};   // H, W
    for (int layout = RELAX_YUV_420P; layout <= RELAX_YUV_NV12; ++layout)
        for (const auto& s : sizes)
            for (int m = 0; m < 4; ++m) {
                if (m && s[0] * s[1] > 64 * 32) continue;          // every matrix and range on the small frames
                geometry(layout, s[0], s[1], m >> 1, m & 1);
            }
    yuv::Plan p;
    const int refused[][3] = {{-1, 4, 4}, {4, 4, 4}, {0, 0, 4}, {0, 4, 0}, {0, -3, 4}, {0, 4, yuv::kMaxDim + 1}, {0, yuv::kMaxDim + 1, 4}};
    const int code[] = {1, 1, 2, 3, 2, 3, 2};
    for (int i = 0; i < 7; ++i)
        if (yuv::plan(refused[i][0], refused[i][1], refused[i][2], &p) != code[i]) fail("refusal code", refused[i][0], refused[i][1], refused[i][2]);
    if (yuv::plan(RELAX_YUV_420P, yuv::kMaxDim, yuv::kMaxDim, &p) != 0 || p.out_bytes != 3LL * yuv::kMaxDim * yuv::kMaxDim ||
        p.frame_bytes != 3LL * yuv::kMaxDim * yuv::kMaxDim / 2)
        fail("largest frame", 0, yuv::kMaxDim, yuv::kMaxDim);
    yuv::Coef k;
    if (yuv::coef(2, 0, &k) || yuv::coef(-1, 1, &k)) fail("matrix accepted", 0, 0, 0);
    std::printf(failures ? "FAILED %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
