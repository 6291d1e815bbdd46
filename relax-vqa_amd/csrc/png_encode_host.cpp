// The encode core of png_deflate.h as plain host C++ (one lane running every virtual thread in turn): the same bytes as the
// device for the same input.  Two builds: librelax_png_encode_host.so (make png_encode_host; the CPU tests encode through
// it and the GPU tests compare the device against it), and, with -DPNG_ENCODE_MAIN, a stand-alone program under
// AddressSanitizer + UBSan (make sanitize_png_encode) that generates its own inputs in exactly sized heap buffers, encodes
// them, inflates the result with the host build of png_inflate.h and compares.  Not part of librelax_hip.so.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "png_deflate.h"
#include "png_inflate.h"

extern "C" int64_t relax_png_encode_bound_host(int H, int W, int C, int filter, int64_t* scratch_bytes, int* band_rows) {
    int64_t scratch = 0, rows = 0;
    const int64_t b = pnge::bound(H, W, C, filter, &scratch, &rows, nullptr, nullptr);
    if (b < 0) return -1;
    if (scratch_bytes) *scratch_bytes = scratch;
    if (band_rows) *band_rows = (int)rows;
    return b;
}

// relax_png_encode on host memory.
extern "C" int relax_png_encode_host(const uint8_t* images, int64_t images_bytes, const int64_t* items, int N, uint8_t* out,
                                     int64_t out_bytes, uint8_t* scratch, int64_t scratch_bytes, int64_t* lengths, int32_t* status) {
    if (N < 0 || images_bytes < 0 || out_bytes < 0 || scratch_bytes < 0 ||
        (N > 0 && (!items || !images || !out || !scratch || !lengths || !status || ((uintptr_t)scratch & 7) ||
                   scratch_bytes < pnge::kPlanHeader + (int64_t)pnge::kPlanEntry * N)))
        return RELAX_ERR_INVALID;
    if (N == 0) return RELAX_OK;
    std::vector<uint64_t> tmp(pnge::kThreads);
    pnge::Shared* s = new pnge::Shared;
    pnge::plan(tmp.data(), items, N, images_bytes, out_bytes, scratch, scratch_bytes, lengths, status);
    const int64_t total = *(const int64_t*)scratch;
    for (int64_t g = 0; g < total; ++g) pnge::encode_band(*s, images, items, N, scratch, g);
    for (int n = 0; n < N; ++n) pnge::place_bands(tmp.data(), items, N, n, out, scratch, lengths, status);
    for (int64_t g = 0; g < total; ++g) pnge::copy_band(items, N, out, scratch, g);
    delete s;
    return RELAX_OK;
}

// The deflate core alone: raw[0, n) (n <= one band) as one band -> a zlib stream in out[0, cap).  -> its length, or -1.
extern "C" int64_t relax_png_deflate_host(const uint8_t* raw, int n, uint8_t* out, int64_t cap) {
    if (!raw || !out || n < 1 || n > pnge::kBandBytes || cap < (int64_t)n + pnge::kBandTail + 6) return -1;
    pnge::Shared* s = new pnge::Shared;
    memcpy(s->f, raw, (size_t)n);
    uint32_t adler = 0;
    const int len = pnge::deflate_band(*s, n, true, out + 2, &adler);
    delete s;
    out[0] = 0x78;
    out[1] = 0x01;
    for (int k = 0; k < 4; ++k) out[2 + len + k] = (uint8_t)(adler >> (24 - 8 * k));
    return 2 + (int64_t)len + 4;
}

#if defined(PNG_ENCODE_MAIN)
namespace {

uint32_t pcg(uint64_t& state) {
    const uint64_t old = state;
    state = old * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t x = (uint32_t)(((old >> 18) ^ old) >> 27), r = (uint32_t)(old >> 59);
    return (x >> r) | (x << ((32 - r) & 31));
}

int failures = 0;
void fail(const char* what, int a, int b, int c, int d) {
    fprintf(stderr, "FAIL %s (%d %d %d %d)\n", what, a, b, c, d);
    ++failures;
}

// kind: 0 constant, 1 horizontal gradient, 2 vertical gradient, 3 noise, 4 zero runs between distinct bytes, 5 smooth + noise
void fill(std::vector<uint8_t>& img, int H, int W, int C, int kind, uint64_t seed) {
    static const int runs[] = {1, 2, 3, 4, 257, 258, 259, 260, 261, 517};
    uint64_t st = seed * 2 + 1;
    const int rb = W * C;
    for (int y = 0; y < H; ++y) {
        int run = 0, left = 0, mark = 1;
        for (int i = 0; i < rb; ++i) {
            uint8_t v = 0;
            if (kind == 0) v = 77;
            else if (kind == 1) v = (uint8_t)((i / C) * 3 + (i % C) * 40);
            else if (kind == 2) v = (uint8_t)(y * 5 + (i % C));
            else if (kind == 3) v = (uint8_t)pcg(st);
            else if (kind == 4) {
                if (left == 0) {
                    v = (uint8_t)(mark++ % 255 + 1);
                    left = runs[(run++ + y) % 10];
                } else {
                    v = 0;
                    --left;
                }
            } else v = (uint8_t)((i / C + y) / 2 + ((pcg(st) & 7) == 0 ? (pcg(st) & 3) : 0));
            img[(size_t)y * rb + i] = v;
        }
    }
}

void check_image(int H, int W, int C, int kind, int filter) {
    const int rb = W * C;
    std::vector<uint8_t> img((size_t)H * rb);
    fill(img, H, W, C, kind, (uint64_t)H * 131 + W * 7 + C + kind);
    int64_t scratch_bytes = 0;
    int rows = 0;
    const int64_t bound = relax_png_encode_bound_host(H, W, C, filter, &scratch_bytes, &rows);
    if (bound < 0) return fail("bound", H, W, C, filter);
    uint8_t* out = (uint8_t*)malloc((size_t)bound);
    uint8_t* scratch = (uint8_t*)malloc((size_t)scratch_bytes);
    memset(scratch, 0xff, (size_t)scratch_bytes);
    int64_t item[8] = {0, rb, H, W, C, 0, bound, filter}, length = -1;
    int32_t status = -1;
    const int rc = relax_png_encode_host(img.data(), (int64_t)img.size(), item, 1, out, bound, scratch, scratch_bytes, &length, &status);
    if (rc != 0 || status != 0 || length < 8 || length > bound) fail("encode", H, W, kind, status);
    else {
        if (kind == 3 && length != bound) fail("noise is not at the bound", H, W, C, (int)(bound - length));
        std::vector<uint8_t> bgr((size_t)H * W * 3), z(out, out + length);     // an exactly sized copy of the stream
        pngd::Shared* d = new pngd::Shared;
        std::vector<uint8_t> raw((size_t)H * (rb + 1));
        const int st = pngd::decode_image(*d, z.data(), length, H, W, C, raw.data(), bgr.data());
        delete d;
        if (st != 0) fail("inflate", H, W, kind, st);
        else
            for (int y = 0; y < H && !failures; ++y)
                for (int x = 0; x < W; ++x)
                    for (int c = 0; c < 3; ++c)
                        if (bgr[((size_t)y * W + x) * 3 + c] != img[(size_t)y * rb + (C == 1 ? x : x * 3 + c)]) {
                            fail("pixels", y, x, c, kind);
                            y = H;
                            x = W;
                            break;
                        }
    }
    free(out);
    free(scratch);
}

void check_raw(const std::vector<uint8_t>& raw, const char* what) {
    const int n = (int)raw.size();
    const int64_t cap = (int64_t)n + pnge::kBandTail + 6;
    uint8_t* out = (uint8_t*)malloc((size_t)cap);
    const int64_t len = relax_png_deflate_host(raw.data(), n, out, cap);
    if (len < 0 || len > cap) fail(what, n, (int)len, 0, 0);
    else {
        std::vector<uint8_t> z(out, out + len), back((size_t)n);
        pngd::Shared* d = new pngd::Shared;
        uint32_t adler = 0;
        const int st = pngd::inflate(*d, z.data(), len, back.data(), n, &adler);
        delete d;
        uint32_t a = 1, b = 0;
        for (int i = 0; i < n; ++i) {
            a = (a + raw[i]) % 65521u;
            b = (b + a) % 65521u;
        }
        if (st != 0 || memcmp(back.data(), raw.data(), (size_t)n) != 0 || adler != ((b << 16) | a)) fail(what, n, st, 1, 0);
    }
    free(out);
}

}  // namespace

int main() {
    static const int shapes[][2] = {{1, 1}, {1, 3}, {5, 3}, {9, 17}, {12, 224}, {224, 224}, {3, 1920}, {2, 5461}};
    int cases = 0;
    for (const auto& hw : shapes)
        for (int C = 1; C <= 3; C += 2)
            for (int kind = 0; kind < 6; ++kind) {
                check_image(hw[0], hw[1], C, kind, -1);
                check_image(hw[0], hw[1], C, kind, (kind + hw[1]) % 5);
                cases += 2;
            }
    for (int C = 1; C <= 3; C += 2) {          // three bands and a shorter last one
        const int W = 700;
        int rows = 0;
        relax_png_encode_bound_host(1, W, C, -1, nullptr, &rows);
        for (int kind = 0; kind < 6; ++kind, ++cases) check_image(2 * rows + (rows + 1) / 2, W, C, kind, kind == 4 ? 0 : -1);
    }
    {   // value k appears F(k) times, k = 1..20, shuffled: a histogram whose Huffman code wants more than 15 bits
        std::vector<uint8_t> raw;
        int f0 = 1, f1 = 1;
        for (int k = 1; k <= 20; ++k) {
            raw.insert(raw.end(), (size_t)f0, (uint8_t)k);
            const int f2 = f0 + f1;
            f0 = f1;
            f1 = f2;
        }
        uint64_t st = 99;
        for (size_t i = raw.size() - 1; i > 0; --i) {
            const size_t j = pcg(st) % (i + 1);
            const uint8_t t = raw[i];
            raw[i] = raw[j];
            raw[j] = t;
        }
        check_raw(raw, "fibonacci");
        // counts w(k) = w(k-1) + w(k-2) + 1 from 2, 4 (no ties: an unlimited Huffman code is 17 deep), no two equal neighbours
        std::vector<uint8_t> sorted;
        {
            int w[17] = {2, 4};
            for (int k = 2; k < 17; ++k) w[k] = w[k - 1] + w[k - 2] + 1;
            for (int k = 16; k >= 0; --k) sorted.insert(sorted.end(), (size_t)w[k], (uint8_t)(k + 1));
        }
        std::vector<uint8_t> spread(sorted.size());
        {
            size_t at = 0;
            for (size_t i = 0; i < spread.size(); i += 2) spread[i] = sorted[at++];
            for (size_t i = 1; i < spread.size(); i += 2) spread[i] = sorted[at++];
        }
        check_raw(spread, "skewed counts, all literals");
        ++cases;
        check_raw(std::vector<uint8_t>(1, 5), "one byte");
        check_raw(std::vector<uint8_t>(2, 5), "two equal bytes");
        check_raw(std::vector<uint8_t>((size_t)pnge::kBandBytes, 0), "a band of zeros");
        std::vector<uint8_t> two(1000);
        for (size_t i = 0; i < two.size(); ++i) two[i] = (uint8_t)(i & 1);
        check_raw(two, "two symbols");
        std::vector<uint8_t> noise((size_t)pnge::kBandBytes);
        for (auto& v : noise) v = (uint8_t)pcg(st);
        check_raw(noise, "noise");
        cases += 6;
    }
    if (failures) {
        printf("png_encode_host: %d FAILED of %d cases\n", failures, cases);
        return 1;
    }
    printf("png_encode_host: OK %d cases\n", cases);
    return 0;
}
#endif
