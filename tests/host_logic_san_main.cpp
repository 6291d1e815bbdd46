// Stand-alone program (its own main) for AddressSanitizer + UBSan: csrc/host_logic.cpp's conv_hoelder and read_bn on the shapes of
// tests/test_conv_hoelder_cpu.py and on malformed BatchNorm dicts, and the options table's set / get with an empty key, a 1 KiB key and every
// key of the table, and vit_plan and vgg_plan on the grids of their CPU tests.  Every input and output sits in a heap block of exactly its size, so a read or write past an end is reported.  Built and run by tests/test_conv_hoelder_cpu.py; exit status 0 and "host_logic_san: OK" if all holds.
#include <cmath>
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

static void hoelder_cases(int cout, int k) {
    std::vector<float> rows((size_t)cout * k), bias((size_t)cout), zeros((size_t)cout * k, 0.f);
    unsigned s = 12345u + (unsigned)cout * 7919u + (unsigned)k;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (float)((int)(s >> 8) % 2001 - 1000) / 512.f; };
    for (float& v : rows) v = next();
    for (float& v : bias) v = next();
    float want_l1 = 0.f, want_b = 0.f;   // the definition, written out once more
    for (int o = 0; o < cout; ++o) {
        double l1 = 0.0;
        for (int j = 0; j < k; ++j) l1 += std::fabs((double)rows[(size_t)o * k + j]);
        want_l1 = std::fmax(want_l1, (float)(l1 * (1.0 + 1e-6)));
        want_b = std::fmax(want_b, std::fabs(bias[(size_t)o]));
    }
    float l1 = -1.f, b = -1.f;
    conv_hoelder(rows.data(), bias.data(), cout, k, &l1, &b);
    CHECK(l1 == want_l1 && b == want_b && l1 > 0.f);
    conv_hoelder(rows.data(), nullptr, cout, k, &l1, &b);
    CHECK(l1 == want_l1 && b == 0.f);
    conv_hoelder(zeros.data(), bias.data(), cout, k, &l1, &b);
    CHECK(l1 == 0.f && b == want_b);
}

static void read_bn_cases() {
    const char* keys[4] = {"weight", "bias", "running_mean", "running_var"};
    const std::string prefix = "layer1.0.bn2";
    std::vector<float> t[4] = {{1.f, -2.f, 0.5f}, {0.25f, 0.f, -1.f}, {0.125f, 3.f, -0.75f}, {1.f, 0.1f, 4.f}};
    std::vector<float> four(4, 0.f), scale(3), shift(3), want_scale(3), want_shift(3);
    std::string err;
    {
        StateDict sd;
        for (int i = 0; i < 4; ++i) sd.add((prefix + "." + keys[i]).c_str(), t[i].data(), 3);
        CHECK(read_bn(sd, prefix, 3, 1e-5f, scale.data(), shift.data(), err) && err.empty());
        fold_bn(t[0].data(), t[1].data(), t[2].data(), t[3].data(), 1e-5f, 3, want_scale.data(), want_shift.data());
        CHECK(scale == want_scale && shift == want_shift);
    }
    for (int missing = 0; missing < 4; ++missing) {
        StateDict sd;
        for (int i = 0; i < 4; ++i)
            if (i != missing) sd.add((prefix + "." + keys[i]).c_str(), t[i].data(), 3);
        err.clear();
        CHECK(!read_bn(sd, prefix, 3, 1e-5f, scale.data(), shift.data(), err));
        CHECK(err.find("missing key '" + prefix + "." + keys[missing] + "'") != std::string::npos);
    }
    for (int bad = 0; bad < 4; ++bad) {   // one key with four values where three are expected; and with a null pointer
        StateDict sd, sd0;
        for (int i = 0; i < 4; ++i) {
            sd.add((prefix + "." + keys[i]).c_str(), i == bad ? four.data() : t[i].data(), i == bad ? 4 : 3);
            sd0.add((prefix + "." + keys[i]).c_str(), i == bad ? nullptr : t[i].data(), 3);
        }
        err.clear();
        CHECK(!read_bn(sd, prefix, 3, 1e-5f, scale.data(), shift.data(), err));
        CHECK(err.find(prefix + "." + keys[bad] + "' has 4 elements, expected 3") != std::string::npos);
        err.clear();
        CHECK(!read_bn(sd0, prefix, 3, 1e-5f, scale.data(), shift.data(), err));
        CHECK(err.find(prefix + "." + keys[bad] + "' has a NULL data pointer") != std::string::npos);
    }
}

// a key in a heap block of exactly its length + 1
static std::vector<char> heap_key(const std::string& k) { return std::vector<char>(k.c_str(), k.c_str() + k.size() + 1); }

static void option_cases() {
    std::vector<relax::GemmOptions> heap(1);   // (the struct in a heap block of its size: a member pointer past its end is reported)
    relax::GemmOptions& o = heap[0];
    const relax::GemmOptions defaults;
    std::string err;
    int v = -7;
    for (const std::string& bad : {std::string(), std::string(1024, 'k')}) {
        const std::vector<char> key = heap_key(bad);
        err.clear();
        CHECK(!option_set(o, key.data(), 1, err) && err == "relax_set_option: unknown option '" + bad + "'");
        err.clear();
        CHECK(!option_get(o, key.data(), &v, err) && err == "relax_get_option: unknown option '" + bad + "'" && v == -7);
    }
    CHECK(!option_set(o, nullptr, 1, err) && err == "relax_set_option: key is NULL");
    CHECK(!option_get(o, nullptr, &v, err) && err == "relax_get_option: NULL argument");
    CHECK(!option_get(o, "gemm_split_k", nullptr, err) && err == "relax_get_option: NULL argument");
    CHECK(std::memcmp(&o, &defaults, sizeof(o)) == 0);
    CHECK(kNumOptions == 20);
    for (int i = 0; i < kNumOptions; ++i) {
        const std::vector<char> key = heap_key(kOptions[i].key);
        int before = -7;
        CHECK(option_get(o, key.data(), &before, err) && before == defaults.*(kOptions[i].member));
        for (const int value : {INT32_MIN, -1, 0, 1, 2, 3, 4, 128, 256, INT32_MAX}) {   // accepted or refused: a refusal leaves the value
            int stored = -7, now = -7;
            CHECK(option_get(o, key.data(), &stored, err));
            err.clear();
            const bool ok = option_set(o, key.data(), value, err);
            CHECK(ok == err.empty());
            CHECK(option_get(o, key.data(), &now, err) && (ok || now == stored));
        }
        CHECK(option_set(o, key.data(), before, err));
    }
    CHECK(std::memcmp(&o, &defaults, sizeof(o)) == 0);
    // the variables: none set, and every one set to a text atoi stops in
    options_from_env(o, [](const char*) -> const char* { return nullptr; });
    CHECK(std::memcmp(&o, &defaults, sizeof(o)) == 0);
    const std::vector<char> text = heap_key("2x");
    options_from_env(o, [&](const char*) -> const char* { return text.data(); });
    CHECK(o.split_k == 2 && o.precision == 2 && o.h2_form == 2 && o.variant == 2 && o.variant_n64 == 2 && o.group_m == 2 && o.debug_poison == 1);
}

// vit_plan on the grid of tests/test_vit_plan_cpu.py (options x widths x patch sizes x token counts x requests): the routes in range, the
// slots in order
static void vit_plan_cases() {
    const int depth = 12, requests[6][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 1, 1, 0}, {0, 0, 0, 1}, {0, 0, 0, depth}};
    for (int precision = 0; precision <= 3; ++precision)
        for (int sw = 0; sw < 4; ++sw)
            for (const int dim : {192, 256, 384, 768})
                for (const int patch : {8, 16})
                    for (const int ntok : {2, 61, 197, 198, 785, 4097})
                        for (const auto& r : requests) {
                            const VitPlan p = vit_plan(VitOptions{precision, sw & 1, sw >> 1}, VitModel{dim, depth, dim / 64, patch, 3 * patch * patch},
                                                       VitRequest{ntok, ntok - 1, r[0], r[1], r[2], r[3]});
                            const VitArena& a = p.arena;
                            CHECK(p.arith >= kVitF32 && p.arith <= kVitH2 && p.attention >= kVitAttention && p.attention <= kVitAttentionStreamH2);
                            CHECK(a.patches == 0 && a.embedded > 0 && a.residual > a.embedded && a.operand > a.residual && a.qkv > a.operand);
                            CHECK(a.final >= a.operand && a.hidden > a.qkv && a.hidden > a.final && a.floats > a.hidden);
                        }
}

// vgg_plan on the grid of tests/test_vgg16_plan_cpu.py (every precision x requests x tap masks x N), accepted at its own slot count and refused
// one short of it: the rows in range, the slots below n_slots, the plan untouched by a refusal.  Every plan sits in a heap block of its size.
static void vgg_plan_cases() {
    const unsigned masks[6] = {0u, 0x7FFFu, 1u << 0, 1u << 3, 1u << 13, 1u << 14};
    for (int precision = 0; precision <= 3; ++precision)
        for (int want = 0; want < 4; ++want)
            for (const unsigned taps : masks)
                for (const int n : {1, kVggChunk}) {
                    if (want == 0 && taps == 0u) continue;
                    const VggRequest rq{n, want & 1, want >> 1, taps};
                    std::vector<VggPlan> heap(1);
                    VggPlan& p = heap[0];
                    std::string err;
                    CHECK(vgg_plan(VggOptions{precision}, rq, kVggSlots, &p, err) && err.empty());
                    CHECK(p.n_slots == (precision == 3 ? 20 : 0) && p.n_rows == (p.classifier ? kVggSteps : kVggSteps - 2));
                    CHECK(p.classifier == (rq.want_pool || (taps >> 13 & 3u)));
                    CHECK(p.arena.a32 == 0 && p.arena.floats == 13054024 && vgg_arena_bytes(n) == 4 * p.arena.floats * n);
                    for (int r = 0; r < p.n_rows; ++r) {
                        const VggLayerPlan& q = p.row[r];
                        CHECK(q.route >= kVggConv11 && q.route <= kVggPoolF32 && q.layer >= 0 && q.layer < kVggTaps);
                        CHECK(q.in >= kVggBufNone && q.in <= kVggBufFc2 && q.out32 >= kVggBufNone && q.out32 <= kVggBufFc2);
                        CHECK(q.out_planes == kVggBufNone || q.out_planes == kVggBufPlanes0 || q.out_planes == kVggBufPlanes1);
                        CHECK(q.s_in < p.n_slots && q.s_out < p.n_slots && q.s_in_max < p.n_slots && q.s_in >= -1 && q.s_out >= -1 && q.s_in_max >= -1);
                        CHECK(q.gap_group == 0 || q.gap_group == 4 || q.gap_group == 16);
                    }
                    std::vector<VggPlan> heap2(1);
                    std::memset(static_cast<void*>(&heap2[0]), 0x5A, sizeof(VggPlan));
                    const VggPlan before = heap2[0];
                    err.clear();
                    CHECK(!vgg_plan(VggOptions{precision}, rq, p.n_slots - 1, &heap2[0], err));
                    CHECK(err == "vgg16: " + std::to_string(p.n_slots) + " per-image scale slots used, " + std::to_string(p.n_slots - 1) + " reserved");
                    CHECK(std::memcmp(&before, &heap2[0], sizeof(VggPlan)) == 0);
                    CHECK(vgg_plan(VggOptions{precision}, rq, p.n_slots, &heap2[0], err));
                }
}

int main() {
    const int shapes[4][2] = {{1, 32}, {3, 64}, {64, 224}, {5, 4608}};
    for (const auto& sh : shapes) hoelder_cases(sh[0], sh[1]);
    read_bn_cases();
    option_cases();
    vit_plan_cases();
    vgg_plan_cases();
    if (failures) return 1;
    std::printf("host_logic_san: OK\n");
    return 0;
}
