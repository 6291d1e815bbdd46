// Stand-alone program (its own main) for AddressSanitizer + UBSan: csrc/host_logic.cpp's ResNet-50 canvas geometry, schedule and stem plan under
// RELAX_RN_CANVAS_ANY - every height and width in [64, 1024] against 64, the canvases of tests/test_resnet_anysize_cpu.py under all option
// settings, and the refusals.  Every output sits in a heap block of exactly its size, so a write past an end is reported.  Built and run by
// tests/test_resnet_anysize_cpu.py; exit status 0 and "rn_anysize_san: OK" if all holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_logic.h"

using namespace relax::host;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

int main() {
    std::vector<RnCanvasGeometry> geo(1);
    std::vector<RnPlan> plan(1);
    std::vector<RnStemPlan> stem(1);
    std::string err;
    auto floor_map = [](int n, int k, int s, int p) { return (n + 2 * p - k) / s + 1; };
    for (int v = kRnCanvasMin; v <= kRnCanvasMax; ++v)
        for (int axis = 0; axis < 2; ++axis) {
            const int Hc = axis ? kRnCanvasMin : v, Wc = axis ? v : kRnCanvasMin;
            err.clear();
            CHECK(rn_canvas_geometry(Hc, Wc, kRnCanvasAny, geo.data(), err) && err.empty());
            const RnCanvasGeometry& g = geo[0];
            const int h0 = floor_map(Hc, 7, 2, 3), w0 = floor_map(Wc, 7, 2, 3), h1 = floor_map(h0, 3, 2, 1), w1 = floor_map(w0, 3, 2, 1);
            CHECK(g.tap_hw[0][0] == h0 && g.tap_hw[0][1] == w0 && g.tap_hw[1][0] == h1 && g.tap_hw[1][1] == w1);
            CHECK(g.big >= (int64_t)h0 * w0 * 64 && g.big >= (int64_t)h1 * w1 * 256 && g.block_max * 256 >= (int64_t)h1 * w1 * 16);
            RnCanvasGeometry old{};
            std::string e2;
            const bool taken = rn_canvas_geometry(Hc, Wc, &old, e2);
            CHECK(taken == (v % kRnCanvasStep == 0) && taken == rn_canvas_default_rule(Hc, Wc));
            CHECK(!taken || std::memcmp(&old, &g, sizeof(g)) == 0);
            RnCanvas cv;
            cv.Hc = Hc; cv.Wc = Wc; cv.flags = kRnCanvasAny;
            CHECK(rn_stem_plan(cv, stem.data(), err));
            CHECK((stem[0].stem_form == kRnStemAny) == !taken && (stem[0].pool_form == kRnPoolAny) == !taken);
            for (const int precision : {2, 3}) {
                CHECK(rn_plan(RnOptions{precision, 1, 1, 1, 1, 1}, RnRequest{40, 15, 15, 1, 0x7fffu}, cv, kRnImgSlots, plan.data(), err));
                for (int b = 0; b < kRnFirstH2Block; ++b) CHECK(precision == 2 || plan[0].blk[b].form != kRnFormX6);
            }
        }
    const int canvases[7][2] = {{65, 67}, {70, 100}, {95, 98}, {230, 232}, {270, 480}, {540, 960}, {1023, 65}};
    for (const auto& c : canvases) {
        RnCanvas cv;
        cv.Hc = c[0]; cv.Wc = c[1]; cv.flags = kRnCanvasAny;
        for (int sw = 0; sw < 32; ++sw)
            for (const int precision : {2, 3})
                CHECK(rn_plan(RnOptions{precision, sw & 1, (sw >> 1) & 1, (sw >> 2) & 1, (sw >> 3) & 1, (sw >> 4) & 1}, RnRequest{4, 4, 0, 1, 0x7fffu}, cv,
                              kRnImgSlots, plan.data(), err));
        cv.flags = 0;
        err.clear();
        CHECK(!rn_plan(RnOptions{3, 1, 1, 1, 1, 1}, RnRequest{4, 4, 0, 1, 0u}, cv, kRnImgSlots, plan.data(), err) && err.find("multiple of 32") != std::string::npos);
    }
    const int bad[5][3] = {{63, 64, kRnCanvasAny}, {64, 1025, kRnCanvasAny}, {0, 64, kRnCanvasAny}, {-5, 64, kRnCanvasAny}, {64, 64, 2}};
    for (const auto& b : bad) {
        std::vector<RnCanvasGeometry> untouched(1);
        std::memset(untouched.data(), 0x5a, sizeof(RnCanvasGeometry));
        const RnCanvasGeometry before = untouched[0];
        err.clear();
        CHECK(!rn_canvas_geometry(b[0], b[1], b[2], untouched.data(), err) && !err.empty());
        CHECK(std::memcmp(&before, untouched.data(), sizeof(before)) == 0);
        CHECK(err.find("(canvas " + std::to_string(b[0]) + " x " + std::to_string(b[1]) + ")") != std::string::npos);
    }
    if (failures) return 1;
    std::printf("rn_anysize_san: OK\n");
    return 0;
}
