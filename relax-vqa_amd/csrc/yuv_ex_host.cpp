// yuv_core.h's RELAX_YUVF_* half on the host, with its own main: the stand-alone program behind `make sanitize_yuv_ex`
// (AddressSanitizer + UBSan, CPU only; tests/test_yuv_ex_cpu.py runs it as a plain child process).  For every format and a list
// of geometries, at an aligned and an unaligned base, it plays every lane of relax_yuv_to_bgr_ex's grid - the bytewise path, and
// the 16-byte path where it applies, with the accesses of fast_unit_ex (memcpy of the access width at the access offset into the
// words yuv::Kind reads) - against heap buffers of exactly frame_bytes and H*W*3 bytes, so an access outside a frame or a slot is
// a sanitizer report.  It checks that the accesses cover every output byte exactly once, that both paths give equal bytes,
// that they equal a conversion written plane by plane, and that at depth 8 pixel_ex is pixel.
// Prints one line per format and geometry (the test compares them with the Python layout) and exits non-zero on any mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "yuv_core.h"

namespace {

int failures = 0;

void fail(const char* what, int format, int H, int W, long long a = 0, long long b = 0) {
    std::printf("MISMATCH %s: format %d H %d W %d (%lld vs %lld)\n", what, format, H, W, a, b);
    ++failures;
}

uint32_t rng_state = 2463534242u;
uint8_t next_byte() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return static_cast<uint8_t>(rng_state >> 24);
}

// heap memory of exactly n bytes whose first byte lies `off` bytes behind a 16-byte boundary: the block is those n bytes and `off`
// canary bytes in front of them, so one byte beyond the buffer is a sanitizer report and a write in front of it is found by check()
struct Heap {
    uint8_t* raw = nullptr;
    uint8_t* at;
    size_t size;
    int off;
    Heap(size_t n, int o) : size(n), off(o) {
        void* m = nullptr;
        if (posix_memalign(&m, 16, n + static_cast<size_t>(o)) != 0) std::abort();
        raw = static_cast<uint8_t*>(m);
        std::memset(raw, 0xA5, static_cast<size_t>(o));
        at = raw + o;
    }
    bool check() const {
        for (int i = 0; i < off; ++i)
            if (raw[i] != 0xA5) return false;
        return true;
    }
    ~Heap() { std::free(raw); }
};

int sample_ref(const yuv::Format& t, const uint8_t* s) {
    const int w = t.sb == 1 ? s[0] : (s[0] | (s[1] << 8));
    return (w >> t.shift) & ((1 << t.depth) - 1);
}

// the conversion written plane by plane from the layout table of include/relax_hip.h, without yuv_core.h's offset functions
void reference(int format, int H, int W, const yuv::Coef& k, const uint8_t* f, uint8_t* o) {
    yuv::Format t;
    yuv::format_traits(format, &t);
    const int cw = (W + (1 << t.hshift) - 1) >> t.hshift, ch = (H + (1 << t.vshift) - 1) >> t.vshift;
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            const int cr = r >> t.vshift, cc = c >> t.hshift;
            const uint8_t *ys, *us, *vs;
            if (t.packing == yuv::kPacked) {
                const uint8_t* grp = f + (static_cast<size_t>(r) * cw + cc) * 4;
                ys = grp + (t.swap ? 1 : 0) + 2 * (c & 1);
                us = grp + (t.swap ? 0 : 1);
                vs = grp + (t.swap ? 2 : 3);
            } else {
                ys = f + (static_cast<size_t>(r) * W + c) * t.sb;
                const uint8_t* cp = f + static_cast<size_t>(H) * W * t.sb;
                if (t.packing == yuv::kSemiPlanar) {
                    const uint8_t* pr = cp + (static_cast<size_t>(cr) * cw + cc) * 2 * t.sb;
                    us = pr + (t.swap ? t.sb : 0);
                    vs = pr + (t.swap ? 0 : t.sb);
                } else {
                    us = cp + (static_cast<size_t>(cr) * cw + cc) * t.sb;
                    vs = us + static_cast<size_t>(ch) * cw * t.sb;
                }
            }
            int b, g, rr;
            yuv::pixel_ex(k, t.depth - 8, sample_ref(t, ys), sample_ref(t, us), sample_ref(t, vs), &b, &g, &rr);
            uint8_t* q = o + (static_cast<size_t>(r) * W + c) * 3;
            q[0] = static_cast<uint8_t>(b), q[1] = static_cast<uint8_t>(g), q[2] = static_cast<uint8_t>(rr);
        }
}

// a lane of the 16-byte path: fast_unit_ex's accesses, yuv::Kind's extraction
template <class K>
void fast_lane(const yuv::Plan& p, int format, const yuv::Coef& k, const uint8_t* f, uint8_t* o, int64_t unit, std::vector<uint8_t>& hits) {
    const yuv::FastUnitEx a = yuv::fast_unit_ex(p, unit);
    if (a.y_bytes != K::kYWords * 4 || a.c_planes != K::kCPlanes || (a.c_planes && a.c_bytes != K::kCBytes) || a.rows > K::kRows)
        return fail("fast_unit_ex and the kernel's kind disagree", format, p.H, p.W, a.y_bytes, a.c_bytes);
    uint32_t lw[K::kRows][K::kYWords], cw[2][K::kCWords];
    std::memset(lw, 0, sizeof lw);
    std::memset(cw, 0, sizeof cw);
    for (int pl = 0; pl < a.c_planes; ++pl) {
        if ((reinterpret_cast<uintptr_t>(f) + a.c[pl]) % a.c_width) fail("misaligned chroma access", format, p.H, p.W, a.c[pl], a.c_width);
        for (int at = 0; at < a.c_bytes; at += a.c_width) std::memcpy(reinterpret_cast<uint8_t*>(cw[pl]) + at, f + a.c[pl] + at, a.c_width);
    }
    for (int j = 0; j < a.rows; ++j) {
        if ((reinterpret_cast<uintptr_t>(f) + a.y[j]) % 16 || (reinterpret_cast<uintptr_t>(o) + a.o[j]) % 16)
            fail("misaligned luma or output access", format, p.H, p.W, a.y[j], a.o[j]);
        for (int at = 0; at < a.y_bytes; at += 16) std::memcpy(reinterpret_cast<uint8_t*>(lw[j]) + at, f + a.y[j] + at, 16);
    }
    const uint32_t* cu = K::kCPlanes == 0 ? lw[0] : cw[0];
    const uint32_t* cv = K::kCPlanes == 0 ? lw[0] : cw[K::kCPlanes == 2 ? 1 : 0];
    for (int j = 0; j < a.rows; ++j) {
        uint8_t px[48];
        for (int i = 0; i < 16; ++i) {
            int b, g, r;
            K::pixel(p, k, lw[j], cu, cv, i, &b, &g, &r);
            px[3 * i] = static_cast<uint8_t>(b), px[3 * i + 1] = static_cast<uint8_t>(g), px[3 * i + 2] = static_cast<uint8_t>(r);
        }
        for (int at = 0; at < 48; at += 16) std::memcpy(o + a.o[j] + at, px + at, 16);
        for (int i = 0; i < 48; ++i) ++hits[static_cast<size_t>(a.o[j]) + i];
    }
}

using Lane = void (*)(const yuv::Plan&, int, const yuv::Coef&, const uint8_t*, uint8_t*, int64_t, std::vector<uint8_t>&);
template <int SB, int PACK, int HS, int VS>
struct LaneOf {   // through yuv::for_kind, the dispatch the kernels use, here with the kinds of formats 0..2 as well
    static Lane get() { return fast_lane<yuv::Kind<SB, PACK, HS, VS>>; }
};

void geometry(int format, int H, int W, int matrix, int full, int base) {
    yuv::Plan p;
    yuv::Coef k;
    if (yuv::plan_ex(format, H, W, &p) != 0 || !yuv::coef(matrix, full, &k)) return fail("plan refused", format, H, W);
    if (base == 0 && matrix == 0 && full == 0)
        std::printf("plan %d %d %d : frame_bytes %lld sb %d depth %d shift %d hshift %d vshift %d packing %d cw %d ch %d y_off %d y_step %d "
                    "y_stride %lld u_off %lld v_off %lld c_step %d c_stride %lld units %lld fast %d\n",
                    format, H, W, static_cast<long long>(p.frame_bytes), p.sb, p.depth, p.shift, p.hshift, p.vshift, p.packing, p.cw, p.ch,
                    p.y_off, p.y_step, static_cast<long long>(p.y_stride), static_cast<long long>(p.u_off), static_cast<long long>(p.v_off),
                    p.c_step, static_cast<long long>(p.c_stride), static_cast<long long>(yuv::units_ex(p)),
                    static_cast<int>(yuv::fast_path(p, 0, 0)));
    // one frame and one slot each in heap memory of exactly frame_bytes and H*W*3 bytes
    Heap src(static_cast<size_t>(p.frame_bytes), base), out(static_cast<size_t>(p.out_bytes), base), fast(static_cast<size_t>(p.out_bytes), base);
    for (size_t i = 0; i < src.size; ++i) src.at[i] = next_byte();
    std::vector<uint8_t> want(static_cast<size_t>(p.out_bytes));
    if (!yuv::item_in_range(p, 0, p.frame_bytes, 0, p.out_bytes) || yuv::item_in_range(p, 1, p.frame_bytes, 0, p.out_bytes) ||
        yuv::item_in_range(p, 0, p.frame_bytes, 1, p.out_bytes) || yuv::item_in_range(p, -1, p.frame_bytes, 0, p.out_bytes))
        fail("item rule", format, H, W);
    reference(format, H, W, k, src.at, want.data());
    std::vector<uint8_t> hits(static_cast<size_t>(p.out_bytes), 0);
    for (int64_t u = 0; u < yuv::units_ex(p); ++u) {
        yuv::unit_bytewise_ex(p, k, src.at, out.at, u);
        const yuv::Unit un = yuv::unit_at_ex(p, u);
        for (int r = un.r0; r < un.r0 + un.rows; ++r)
            for (int c = un.c0; c < un.c0 + un.cols; ++c)
                for (int q = 0; q < 3; ++q) ++hits[static_cast<size_t>(yuv::out_at(p, r, c)) + q];
    }
    for (size_t i = 0; i < hits.size(); ++i)
        if (hits[i] != 1) {
            fail("bytewise: an output byte written other than once", format, H, W, static_cast<long long>(i), hits[i]);
            break;
        }
    if (std::memcmp(out.at, want.data(), want.size())) fail("bytewise path differs from the plane-by-plane conversion", format, H, W);
    const bool is_fast = yuv::fast_path(p, reinterpret_cast<uint64_t>(src.at), reinterpret_cast<uint64_t>(fast.at));
    if (is_fast != (W % 16 == 0 && base % 16 == 0)) fail("fast_path condition", format, H, W, is_fast, base);
    if (is_fast) {
        std::fill(hits.begin(), hits.end(), 0);
        const Lane lane = yuv::for_kind<LaneOf, true>(p);
        if ((yuv::for_kind<LaneOf, false>(p) == nullptr) != (format <= RELAX_YUVF_444P)) fail("kinds without a kernel", format, H, W);
        for (int64_t u = 0; u < yuv::units_ex(p); ++u) lane(p, format, k, src.at, fast.at, u, hits);
        for (size_t i = 0; i < hits.size(); ++i)
            if (hits[i] != 1) {
                fail("16-byte path: an output byte written other than once", format, H, W, static_cast<long long>(i), hits[i]);
                break;
            }
        if (std::memcmp(fast.at, out.at, want.size())) fail("16-byte path differs from the bytewise path", format, H, W);
    }
    if (!src.check() || !out.check() || !fast.check()) fail("a byte in front of a buffer was written", format, H, W);
}

}  // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {2, 2}, {7, 5}, {17, 33}, {18, 34}, {36, 64}, {2, 16}, {5, 16}, {7, 48}, {32, 64}, {3, 32}, {131, 97}};   // H, W
    for (int format = 0; format < RELAX_YUVF_COUNT; ++format)
        for (const auto& s : sizes)
            for (int base : {0, 1, 2})
                for (int m = 0; m < 4; ++m) {
                    if (m && s[0] * s[1] > 64 * 36) continue;          // every matrix and range on the small frames
                    geometry(format, s[0], s[1], m >> 1, m & 1, base);
                }
    // at depth 8 the one formula is relax_yuv_to_bgr's, on every (Y, U, V) of a coarse grid and the ends
    for (int m = 0; m < 4; ++m) {
        yuv::Coef k;
        yuv::coef(m >> 1, m & 1, &k);
        for (int Y = 0; Y < 256; ++Y)
            for (int U = 0; U < 256; U += (U % 16 == 15 ? 1 : 3))
                for (int V = 0; V < 256; V += (V % 16 == 15 ? 1 : 3)) {
                    int a[3], b[3];
                    yuv::pixel(k, Y, U, V, &a[0], &a[1], &a[2]);
                    yuv::pixel_ex(k, 0, Y, U, V, &b[0], &b[1], &b[2]);
                    if (a[0] != b[0] || a[1] != b[1] || a[2] != b[2]) fail("pixel_ex at depth 8 is not pixel", m, Y, U, V);
                }
    }
    yuv::Plan p, q;
    for (int layout = 0; layout < 4; ++layout) {                       // plan() is formats 0..3 of plan_ex
        if (yuv::plan(layout, 17, 33, &p) != 0 || yuv::plan_ex(layout, 17, 33, &q) != 0 || p.frame_bytes != q.frame_bytes || p.u_off != q.u_off ||
            p.v_off != q.v_off || p.c_step != q.c_step || p.c_stride != q.c_stride || p.cw != q.cw || p.ch != q.ch)
            fail("plan and plan_ex disagree", layout, 17, 33);
    }
    const int refused[][3] = {{-1, 4, 4}, {RELAX_YUVF_COUNT, 4, 4}, {9, 0, 4}, {9, 4, 0}, {6, 4, yuv::kMaxDim + 1}, {6, yuv::kMaxDim + 1, 4}};
    const int code[] = {1, 1, 2, 3, 3, 2};
    for (int i = 0; i < 6; ++i)
        if (yuv::plan_ex(refused[i][0], refused[i][1], refused[i][2], &p) != code[i]) fail("refusal code", refused[i][0], refused[i][1], refused[i][2]);
    if (yuv::plan(4, 4, 4, &p) != 1) fail("plan accepted a layout beyond NV12", 4, 4, 4);
    std::printf(failures ? "FAILED %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
